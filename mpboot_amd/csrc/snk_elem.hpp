// snk_elem.hpp -- the element type of the weighted (Sankoff) kernels, shared by kernels.hip and place.hip (device code only).
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

}  // namespace mpf
