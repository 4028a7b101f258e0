// Packed int4 weight codes (paddle_amd.quantization.weight_quantize,
// "weight_only_int4"), shared by the int4 decode streamer and the
// dequantizer:
//   qw    int8 [K/2, N] row-major; byte (kp, n) = (q[2kp, n] & 0xF) |
//         ((q[2kp+1, n] & 0xF) << 4), two's-complement nibbles, codes -7..7
//   scale fp32 [N] (per channel) or [K/gs, N] (groups of gs k rows)
//   w[k, n] ~ q[k, n] * scale[k / gs, n] / 7
#pragma once

#include "common.h"

namespace pa {

// low / high nibble of byte `j` (0..3) of a dword, sign-extended
__device__ __forceinline__ int q4_lo(unsigned w, int j) { return (int)(w << (28 - 8 * j)) >> 28; }
__device__ __forceinline__ int q4_hi(unsigned w, int j) { return (int)(w << (24 - 8 * j)) >> 28; }

// log2 of the group size, -1 for per-channel scales
inline int group_shift(int64_t group_size) {
  return group_size == 64 ? 6 : (group_size == 128 ? 7 : -1);
}

}  // namespace pa
