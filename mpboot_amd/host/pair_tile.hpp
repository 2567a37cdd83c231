// pair_tile.hpp -- the tile shapes of the pair products (k_place_costs, place.hip; k_tbr_costs, tbr.hip), one table.  Device-free
// plain C++17: csrc/place.hpp instantiates the kernels from it, host/tbr_plan.hpp cuts a visit's matrix into items with it.
//
// A workgroup of 256 lanes owns TQ rows x TB columns of outputs (placement: queries x branches; TBR: F x G of one visit) and walks
// the operand rows in slices of KS elements (words of 32 sites; on the weighted engine patterns, or pairs of patterns in the 16-bit
// store); a lane holds RQ x RB outputs and, in the narrow shape, one of KT interleaved element classes of a slice (summed through LDS
// at the end: no atomics).
//   wide   (many rows):     4 state rows: 64 x 64, 4 x 4 per lane, KS 16;   32 state rows: 32 x 32, 2 x 2 per lane, KS 4;
//                           20 state rows: the 32-row shape, on the weighted engine 64 x 64, 4 x 4 per lane, KS 4
//   narrow (few outputs, every computeParsimonyTree step): 4 rows x 16 columns, 4 x 1 per lane, KT = KS = 16
// DESIGN 5p has the measurements behind the numbers.
#pragma once

namespace mpf {

enum { PLACE_AUTO = 0, PLACE_NARROW = 1, PLACE_WIDE = 2 };      // the values of the options "place_tile" and "tbr_tile"
struct PlaceShape { int tq, tb, rq, rb, ks, kt; };
constexpr PlaceShape place_shape(int S, bool weighted, int tile)      // tile: PLACE_NARROW | PLACE_WIDE
{
  if (tile == PLACE_NARROW) return PlaceShape{4, 16, 4, 1, 16, 16};
  if (S == 4) return PlaceShape{64, 64, 4, 4, 16, 1};
  return S == 20 && weighted ? PlaceShape{64, 64, 4, 4, 4, 1} : PlaceShape{32, 32, 2, 2, 4, 1};
}

}  // namespace mpf
