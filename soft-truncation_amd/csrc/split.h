// split.h -- the fp16 two-way split rule, once, for every kernel that produces or consumes split operands: the split
// convolutions (conv_x2.h, conv_pl.h), the attention kernels (attention.hip, attention_long.hip) and the GroupNorm kernels
// that write planes (groupnorm.hip).
//
// An operand tensor is multiplied by the power of two s that puts its |x| bound in [2^13, 2^14) (pow2_scale_of: exact,
// undone exactly by the consumer's epilogue); a scaled value v becomes hi = fp16(v), lo = fp16(v - hi), both rounded to
// nearest even; two neighbours share a 32-bit word, the first in its low half (pack_h2).  Every fp16-mode, planes and
// attention tolerance of the tests assumes that all producers follow this one rule.
//
// Conversions, one exact subtraction and bit moves only: nothing here may hold a multiply-add.  A file that switches
// contraction off does so with a pragma that holds "for every function that follows" it, and this header is included
// before any such pragma (the reason stream.h gives for itself), so a product feeding a sum written here would be compiled
// under another rule than the including file states.  Callers scale their values before they call.
//
// namespace split2 ("two-way split"; attention_long.hip has a host function called split): a file with many call sites
// brings the names in with using-declarations in its own namespace.
#pragma once
#include "common.h"

typedef _Float16 halfx2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace split2 {

// power of two s with m * s in [2^13, 2^14) (1 for m = 0)
__device__ __forceinline__ float pow2_scale_of(float m) {
  const int be = (int)((__float_as_uint(m) >> 23) & 0xffu);          // m = 1.f * 2^(be - 127)
  if (be == 0) return 1.f;
  const int se = min(max(127 + 13 - (be - 127), 1), 254);
  return __uint_as_float((unsigned)se << 23);
}
__device__ __forceinline__ unsigned pack_h2(float lo, float hi) {
  const halfx2 v = {(_Float16)lo, (_Float16)hi};                      // round to nearest even
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float lo_part(float v) { return v - (float)(_Float16)v; }   // exact

// four scaled fp32 values -> hi and lo fp16 quadruples (8 bytes each)
__device__ __forceinline__ void split4(const float (&v)[4], u32x2& hi, u32x2& lo) {
  hi = u32x2{pack_h2(v[0], v[1]), pack_h2(v[2], v[3])};
  lo = u32x2{pack_h2(lo_part(v[0]), lo_part(v[1])), pack_h2(lo_part(v[2]), lo_part(v[3]))};
}
// eight scaled fp32 values (8 consecutive channels of one pixel) -> the 16 bytes of the hi and of the lo plane
__device__ __forceinline__ void split8(const float (&v)[8], u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    hi[j] = pack_h2(v[2 * j], v[2 * j + 1]);
    lo[j] = pack_h2(lo_part(v[2 * j]), lo_part(v[2 * j + 1]));
  }
}

}  // namespace split2
