// appnp_topk_key.h -- the total order of the top-k selections and the wave-level
// digit search of their radix selects, shared by appnp_topk_columns (appnp_topk.hip) and
// appnp_push_topk (appnp_push.hip).
//
// Internal to libppnp_amd.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "appnp_device.h"  // kWave

namespace appnp {

// The order-preserving uint32 image of an fp32 candidate: -0 folded onto +0, every NaN mapped to
// 0, below the image of -inf.  A larger key is a better candidate.
__device__ __forceinline__ uint32_t order_key(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;   // NaN: below every number
  if ((u & 0x7fffffffu) == 0u) u = 0u;              // -0 == +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr uint32_t kOrderKeyZero = 0x80000000u;  // order_key(+0.0f): v > 0 iff its key is larger

// One pass of a radix select, by a whole wave: lane l holds the counts h0..h3 of the bins 4 l ..
// 4 l + 3 of a 256-bin histogram of digits, and the want-th largest key is looked for
// (1 <= want <= the histogram's total).  True in exactly one lane, which gets the digit whose bin
// holds that key, the keys in the bins above it and the keys in it.
__device__ __forceinline__ bool digit_search(uint32_t h0, uint32_t h1, uint32_t h2, uint32_t h3,
                                             uint32_t want, int lane, uint32_t& digit,
                                             uint32_t& above, uint32_t& in) {
  const uint32_t own = h0 + h1 + h2 + h3;
  uint32_t suf = own;  // inclusive suffix sum over lanes >= lane
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t t = __shfl_down(suf, off, kWave);
    if (lane + off < kWave) suf += t;
  }
  above = suf - own;  // keys in the bins of higher lanes
  if (!(above < want && want <= suf)) return false;
  uint32_t d = 3;  // the lane's bins from the top: the first whose running count reaches want
  in = h3;
  if (above + h3 < want) {
    above += h3; d = 2; in = h2;
    if (above + h2 < want) {
      above += h2; d = 1; in = h1;
      if (above + h1 < want) { above += h1; d = 0; in = h0; }
    }
  }
  digit = 4u * lane + d;
  return true;
}

}  // namespace appnp
