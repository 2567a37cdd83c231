// wave_min.hpp -- the first minimum of a wave of 64 lanes, "lowest value, lowest index among equals" (k_place_best, k_tbr_best).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpf {

// Every lane brings (v, at), its lowest value and the lowest index that has it, and gets the wave's: a lane takes the other lane's
// pair when its value is lower, or equal with a lower index.  A lane that has seen no entry brings (0xFFFFFFFF, (I)-1): the largest
// pair there is, so it loses to every entry and only a wave of such lanes ends with it.
template <class I> struct MinAt { uint32_t v; I at; };
template <class I>
__device__ __forceinline__ MinAt<I> wave_first_min(uint32_t v, I at)
{
  static_assert(sizeof(I) == 4 || sizeof(I) == 8, "a 32-bit or a 64-bit index");
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t ov = (uint32_t)__shfl_xor((int)v, off, 64);
    I oat = (I)(uint32_t)__shfl_xor((int)(uint32_t)at, off, 64);
    if constexpr (sizeof(I) == 8) oat |= (I)(uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)at >> 32), off, 64) << 32;
    if (ov < v || (ov == v && oat < at)) { v = ov; at = oat; }
  }
  return MinAt<I>{v, at};
}

}  // namespace mpf
