// snk_elem.hpp -- the element type of the weighted (Sankoff) kernels and a lane's min-plus transform, shared by kernels.hip, place.hip
// and tbr.hip (device code only).
//
// PK = false: one 32-bit cost per lane (any cost matrix); PK = true: two 16-bit costs per lane (v_pk_add_u16 / v_pk_min_u16: the
// reference's default "short" arithmetic, usable while 3 n (max cost + 1) < 65536, Engine::pack), half the instructions and half
// the bytes per pattern.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace mpf {

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

template <bool PK> struct SnkT;
template <> struct SnkT<false> {
  typedef uint32_t E;
  static __device__ __forceinline__ E add(E a, E b) { return a + b; }
  static __device__ __forceinline__ E mn(E a, E b) { return min(a, b); }
  static __device__ __forceinline__ E cst(uint32_t c) { return c; }
  static __device__ __forceinline__ E inf() { return 0xFFFFFFFFu; }
  static __device__ __forceinline__ uint32_t sum(E a) { return a; }
  static __device__ __forceinline__ uint32_t wsum(E a, const uint32_t *__restrict__ pwgt, int e) { return a * pwgt[e]; }
};
template <> struct SnkT<true> {
  typedef us2 E;
  static __device__ __forceinline__ E add(E a, E b) { return a + b; }
  static __device__ __forceinline__ E mn(E a, E b) { return __builtin_elementwise_min(a, b); }
  static __device__ __forceinline__ E cst(uint32_t c) { return __builtin_bit_cast(us2, c); }
  static __device__ __forceinline__ E inf() { return (us2){0xFFFF, 0xFFFF}; }
  static __device__ __forceinline__ uint32_t sum(E a) { return (uint32_t)a.x + (uint32_t)a.y; }
  static __device__ __forceinline__ uint32_t wsum(E a, const uint32_t *__restrict__ pwgt, int e)
  {
    return (uint32_t)a.x * pwgt[2 * e] + (uint32_t)a.y * pwgt[2 * e + 1];
  }
};

// ---- a lane's vector and its min-plus transform (kernels.hip: the weighted scan, NNI and view kernels; tbr.hip: the root sets)

template <int S, bool PK>
struct Costs { typename SnkT<PK>::E v[S]; };

// We = elements per state row (Wp patterns, or Wp / 2 pairs); a vector is S rows of We elements
template <int S, bool PK>
__device__ __forceinline__ void load_costs(Costs<S, PK> &t, const uint32_t *__restrict__ vec, uint32_t slot, int We, int e0)
{
  const typename SnkT<PK>::E *p = reinterpret_cast<const typename SnkT<PK>::E *>(vec) + (size_t)slot * (size_t)(S * We) + e0;
#pragma unroll
  for (int k = 0; k < S; k++) t.v[k] = p[(size_t)k * We];
}

// m[z] = min_x(v[x] + cost[z][x]), four z at a time: four independent add -> min chains side by side (a dependent
// packed-math pair costs a wait state), each reading its row of the matrix through the scalar cache.
template <int S, bool PK>
__device__ __forceinline__ void mplus(Costs<S, PK> &m, const Costs<S, PK> &v, const uint32_t *__restrict__ cost)
{
  typedef SnkT<PK> T;
  static_assert(S % 4 == 0, "state count must be a multiple of 4");
#pragma unroll
  for (int z0 = 0; z0 < S; z0 += 4) {
    typename T::E a0 = T::add(v.v[0], T::cst(cost[(z0 + 0) * S])), a1 = T::add(v.v[0], T::cst(cost[(z0 + 1) * S]));
    typename T::E a2 = T::add(v.v[0], T::cst(cost[(z0 + 2) * S])), a3 = T::add(v.v[0], T::cst(cost[(z0 + 3) * S]));
#pragma unroll
    for (int x = 1; x < S; x++) {
      const typename T::E t0 = T::add(v.v[x], T::cst(cost[(z0 + 0) * S + x])), t1 = T::add(v.v[x], T::cst(cost[(z0 + 1) * S + x]));
      const typename T::E t2 = T::add(v.v[x], T::cst(cost[(z0 + 2) * S + x])), t3 = T::add(v.v[x], T::cst(cost[(z0 + 3) * S + x]));
      a0 = T::mn(a0, t0); a1 = T::mn(a1, t1); a2 = T::mn(a2, t2); a3 = T::mn(a3, t3);
    }
    m.v[z0] = a0; m.v[z0 + 1] = a1; m.v[z0 + 2] = a2; m.v[z0 + 3] = a3;
  }
}

// The 16-bit form of the transform on a PAIR-PACKED matrix (round 6): the device copy of the cost matrix carries, behind its S x S
// replicated entries (c | c << 16), S x S / 2 words holding two neighbouring entries of a row each (c[z][2j] | c[z][2j + 1] << 16);
// VOP3P's op_sel picks which half of the scalar operand feeds BOTH halves of the packed add, so a group of four rows needs 40
// scalar registers instead of 80 -- the matrix operand of the next group can be on its way while this one is combined (with 80 of
// the ~100 scalar registers tied up per group the loads could not run ahead: the transform waited on the scalar cache for about
// as long as its 780 packed operations took, profiles/r3/valu_rate.txt).
// (written as shuffles of the scalar word: the instruction selector folds them into the packed add's op_sel / op_sel_hi bits --
//  inline asm for the same instruction kept the compiler from scheduling around it and cost 1.2 KB of scratch per lane)
__device__ __forceinline__ us2 pk_add_lo(us2 v, uint32_t c2) { const us2 p = __builtin_bit_cast(us2, c2); return v + __builtin_shufflevector(p, p, 0, 0); }
__device__ __forceinline__ us2 pk_add_hi(us2 v, uint32_t c2) { const us2 p = __builtin_bit_cast(us2, c2); return v + __builtin_shufflevector(p, p, 1, 1); }
template <int S>
__device__ __forceinline__ void mplus(Costs<S, true> &m, const Costs<S, true> &v, const uint32_t *__restrict__ cost, int /* pair-packed */)
{
  typedef SnkT<true> T;
  static_assert(S % 4 == 0, "state count must be a multiple of 4");
  const uint32_t *__restrict__ c2 = cost + S * S;
  constexpr int H = S / 2;
#pragma unroll
  for (int z0 = 0; z0 < S; z0 += 4) {
    us2 a0, a1, a2, a3;
#pragma unroll
    for (int j = 0; j < H; j++) {
      const uint32_t w0 = c2[(z0 + 0) * H + j], w1 = c2[(z0 + 1) * H + j], w2 = c2[(z0 + 2) * H + j], w3 = c2[(z0 + 3) * H + j];
      const us2 t0 = pk_add_lo(v.v[2 * j], w0), t1 = pk_add_lo(v.v[2 * j], w1), t2 = pk_add_lo(v.v[2 * j], w2), t3 = pk_add_lo(v.v[2 * j], w3);
      if (j == 0) { a0 = t0; a1 = t1; a2 = t2; a3 = t3; }
      else { a0 = T::mn(a0, t0); a1 = T::mn(a1, t1); a2 = T::mn(a2, t2); a3 = T::mn(a3, t3); }
      const us2 u0 = pk_add_hi(v.v[2 * j + 1], w0), u1 = pk_add_hi(v.v[2 * j + 1], w1), u2 = pk_add_hi(v.v[2 * j + 1], w2), u3 = pk_add_hi(v.v[2 * j + 1], w3);
      a0 = T::mn(a0, u0); a1 = T::mn(a1, u1); a2 = T::mn(a2, u2); a3 = T::mn(a3, u3);
    }
    m.v[z0] = a0; m.v[z0 + 1] = a1; m.v[z0 + 2] = a2; m.v[z0 + 3] = a3;
  }
}
// (the scan kernels' call: pair-packed for the 16-bit form, the plain matrix otherwise)
template <int S, bool PK>
__device__ __forceinline__ void mplus_fast(Costs<S, PK> &m, const Costs<S, PK> &v, const uint32_t *__restrict__ cost)
{
  if constexpr (PK) mplus<S>(m, v, cost, 0);
  else mplus<S, PK>(m, v, cost);
}

}  // namespace mpf
