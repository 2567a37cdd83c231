// place.hpp -- launch interface of the taxon-insertion kernels (place.hip; host/place.cpp).
//
// addTaxonMPFast (phylotree.cpp:1322-1378) tries a taxon on every branch of a tree; the length of the tree with query tip T in
// the middle of a branch whose two directed views are A and B is len(tree) + #sites where X and T share no state, X = A & B where
// that is non-empty, else A | B.  For Q queries and B branches that is a Q x B x row-words popcount product.
#pragma once
#include "kernels.hpp"
#include "../host/pair_tile.hpp"

namespace mpf {

// The tile shapes of k_place_costs -- PlaceShape, place_shape(S, weighted, tile), PLACE_AUTO | PLACE_NARROW | PLACE_WIDE -- are in
// host/pair_tile.hpp, the one table that the TBR pair product (tbr.hip, host/tbr_plan.hpp) reads too; DESIGN 5p.
// PLACE_AUTO -> the narrow shape below `narrow_below` outputs (queries x branches), the wide one from there on
int place_pick(int n_query, int n_br, int tile, long long narrow_below);
long long place_narrow_below();                     // the Fitch engine's line: 2^18

// delta[q * ld + b] = #sites (weight-replicated) at which branch b = (desc[b].a, desc[b].b: slots of its two directed views, a
// tip's own vector at a pendant branch) joined as above shares no state with the vector in slot qslot[q].  Row-major store only.
hipError_t launch_place_costs(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br,
                              const uint32_t *qslot, int n_query, uint32_t *delta, int ld, int tile);
// The weighted (-cost) engine.  out[q * ld + b] = the FULL weighted length of the tree with the tip in slot
// qslot[q] in the middle of branch b, evaluated at the new tip's edge (parstree.cpp:439-541, the tip the transformed side):
//   sum_ptn w * min_i( m(T_q)[i] + m(A_b)[i] + m(B_b)[i] ),   m(v) the stored transform `g.moff` words behind v, A, B = desc[b].a, .b
// The same kernel over the min-plus algebra, rows of We = Wp (32-bit store) or Wp / 2 (16-bit store, two patterns per operation) elements.
// wide_addr: 64-bit element offsets (always taken when a half of the store is 4 GiB or more)
// PLACE_AUTO -> narrow below this many outputs (queries x branches).  Both shapes' times grow with the row length alike, so the
// line is a number of outputs; measured on C3 (profiles/place/timing_weighted.json): the 16-bit store crosses near 3.5e5,
// the 32-bit store near 2.45e5; 20 rows on a 1200 x 1000 protein input with 768 taxa held out: near 3.4e5 and 2.75e5.  32 rows were
// not measured and take the 20-row lines
long long place_snk_narrow_below(int S, bool packed);
hipError_t launch_snk_place_costs(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br,
                                  const uint32_t *qslot, int n_query, uint32_t *out, int ld, int tile, bool wide_addr);
// best[2 q] = min_b delta[q * ld + b], best[2 q + 1] = the lowest b that has it (one wave per query)
hipError_t launch_place_best(hipStream_t st, const uint32_t *delta, int n_br, int n_query, int ld, uint32_t *best);

// my_random_shuffle over the identity on the stream handed over by state (placetree::shuffle_order, host/place_tree.hpp)
void place_shuffle_order(int n, uint64_t *state, int32_t *order);

}  // namespace mpf
