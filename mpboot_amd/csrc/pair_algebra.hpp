// pair_algebra.hpp -- the two algebras of the pair products (k_place_costs, place.hip; k_tbr_costs, tbr.hip): device code only.
//
// Both kernels are one tile-product skeleton (the shapes: host/pair_tile.hpp) written over an algebra A, which supplies what the two
// engines do differently.  k_tbr_costs reads absolute row pointers and has no join: it uses S, NP, E, slice_ok, mul, add, weigh, finish.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "snk_elem.hpp"

namespace mpf {

// An algebra of k_place_costs:
//   S, Off          state rows; the type of an element offset from the row base the launcher hands over
//   NP              pattern weights per element that ride along with a slice (0: no weight slice is staged)
//   slice_ok<KS>    what the algebra asks of the slice length besides the skeleton's own conditions
//   join            the S rows of the branch operand (x[s ld], in LDS) from those of its two views (all S rows of both are there before
//                   any is written)
//   mul, add        the product of a query and a branch element; the sum of two products (a lane's first product starts the sum)
//   weigh           what element k of the slice adds to an output (sw: the slice's weights)
//   finish          the output from the sum over a row of `len` elements
template <int S_>
struct PlaceFitch {
  static constexpr int S = S_, NP = 0;
  typedef size_t Off;
  typedef const uint32_t *Row;                       // 64-bit pointers
  typedef uint32_t E;
  template <int KS> static constexpr bool slice_ok = true;
  static __device__ __forceinline__ Row row(const uint32_t *base, Off at) { return base + at; }
  static __device__ __forceinline__ uint32_t load(const uint32_t *, Row r, Off s, Off k) { return r[s + k]; }
  static __device__ __forceinline__ uint32_t gather(uint32_t any, uint32_t a, uint32_t b) { return any | (a & b); }
  static __device__ __forceinline__ uint32_t join(uint32_t any, uint32_t a, uint32_t b) { return (a & b) | (~any & (a | b)); }
  static __device__ __forceinline__ E mul(E q, E x) { return q & x; }
  static __device__ __forceinline__ E add(E m, E t) { return m | t; }
  static __device__ __forceinline__ uint32_t weigh(E m, const uint32_t *, int) { return (uint32_t)__popc(m); }
  static __device__ __forceinline__ uint32_t finish(uint32_t acc, uint32_t bits) { return bits - acc; }
};

// On a ParsTree addTaxonMPFast's score is the FULL length of the completed tree evaluated at the new taxon's edge
// (computeParsimonyBranch(added_node->neighbors[0], added_node), parstree.cpp:439-541; the leaf swap at :449-457 makes the taxon
// the transformed side, the rest of the tree the rows of the matrix).  With A, B the two directed views of the branch and T the
// taxon's cost row, m() the min-plus transform with the viewer as the parent:
//   cost(q, b) = sum_ptn w * min_i( m(T_q)[i] + m(A_b)[i] + m(B_b)[i] )
// All three transforms are STORED (k_poly_snk_views and k_snk_pack write m(v) `moff` words behind v), so nothing is transformed
// here.  16-bit store: a sum of three transforms over disjoint sides that hold at most n tips together -- the shape Engine::pack
// guards (3 n highest_cost < 65536).
//
// The row has We elements (patterns, or pairs of patterns in the 16-bit store); the branch operand is loaded as the two transforms
// and ADDED on the way into LDS, so m(A) + m(B) never exists in HBM; the slice's pattern weights ride along.  Per (query, branch,
// element) a lane does S add / min pairs (v_pk_add_u16 / v_pk_min_u16 in the 16-bit store: two patterns each) and one weighted
// sum.  Padding elements have weight 0.  The element type is SnkT<PK> of the other weighted kernels (snk_elem.hpp).
// BIG: 64-bit element offsets (a transform half of 4 GiB or more); otherwise 32-bit offsets from the half's base
template <int S_, bool PK, bool BIG>
struct PlaceMinPlus {
  typedef SnkT<PK> T;
  static constexpr int S = S_, NP = PK ? 2 : 1;
  typedef typename std::conditional<BIG, size_t, uint32_t>::type Off;
  typedef Off Row;                                   // offsets from the half's base
  typedef typename T::E E;
  template <int KS> static constexpr bool slice_ok = 16 % KS == 0 && KS * NP <= 256;     // a row is whole slices; one lane per weight of a slice
  static __device__ __forceinline__ Row row(const uint32_t *, Off at) { return at; }
  static __device__ __forceinline__ uint32_t load(const uint32_t *base, Row r, Off s, Off k) { return base[r + s + k]; }
  static __device__ __forceinline__ uint32_t gather(uint32_t, uint32_t, uint32_t) { return 0u; }
  static __device__ __forceinline__ uint32_t join(uint32_t, uint32_t a, uint32_t b)
  {
    return __builtin_bit_cast(uint32_t, T::add(__builtin_bit_cast(E, a), __builtin_bit_cast(E, b)));
  }
  static __device__ __forceinline__ E mul(E q, E x) { return T::add(q, x); }
  static __device__ __forceinline__ E add(E m, E t) { return T::mn(m, t); }
  static __device__ __forceinline__ uint32_t weigh(E m, const uint32_t *sw, int k) { return T::wsum(m, sw, k); }
  static __device__ __forceinline__ uint32_t finish(uint32_t acc, uint32_t) { return acc; }
};

}  // namespace mpf
