// appnp_topk_key.h -- the total order of the top-k selections, shared by
// appnp_topk_columns (appnp_topk.hip) and appnp_push_topk (appnp_push.hip).
//
// Internal to libppnp_amd.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace appnp
