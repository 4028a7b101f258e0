// Weight-only int4 dequantizer: packed [K/2, N] + scales -> bf16 | fp32
// [K, N] (storage format: int4_codes.h).  Used by weight_only_linear for
// rows > 32 and by paddle.nn.quant.weight_dequantize; the decode streamer
// for rows <= 32 is decode_gemm.hip.
#include "common.h"
#include "api.h"
#include "int4_codes.h"

namespace pa {

namespace {

// Dequantize 8 columns of one packed row (= 2 k rows) per thread.  Every
// element is evaluated as  float(q) * (scale * C7)  with C7 = fp32(1/7):
// two correctly rounded fp32 multiplies, kept in that order.
template <bool BF16OUT>
__global__ void dequant_int4_kernel(const signed char* __restrict__ wq,
                                    const float* __restrict__ scale,
                                    void* __restrict__ out, long long kp_rows,
                                    long long N, int gshift) {
#pragma clang fp reassociate(off) contract(off)
  const long long nseg = N >> 3;
  const long long total = kp_rows * nseg;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long kp = i / nseg;
    const long long n = (i % nseg) << 3;
    const uint2 b = *reinterpret_cast<const uint2*>(wq + kp * N + n);
    const unsigned bw[2] = {b.x, b.y};
    const long long g = gshift < 0 ? 0 : ((2 * kp) >> gshift);
    const float* sp = scale + g * N + n;
    float lo[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float s7 = sp[j] * (1.f / 7.f);
      lo[j] = (float)q4_lo(bw[j >> 2], j & 3) * s7;
      hi[j] = (float)q4_hi(bw[j >> 2], j & 3) * s7;
    }
    const long long o0 = (2 * kp) * N + n, o1 = o0 + N;
    if (BF16OUT) {
      *reinterpret_cast<shortx8*>((short*)out + o0) = f8_to_bf8(lo);
      *reinterpret_cast<shortx8*>((short*)out + o1) = f8_to_bf8(hi);
    } else {
      float4* p0 = reinterpret_cast<float4*>((float*)out + o0);
      float4* p1 = reinterpret_cast<float4*>((float*)out + o1);
      p0[0] = float4{lo[0], lo[1], lo[2], lo[3]};
      p0[1] = float4{lo[4], lo[5], lo[6], lo[7]};
      p1[0] = float4{hi[0], hi[1], hi[2], hi[3]};
      p1[1] = float4{hi[4], hi[5], hi[6], hi[7]};
    }
  }
}

}  // namespace

void dequant_int4(const void* qw, const float* scale, void* out, int64_t k,
                  int64_t n, int64_t group_size, int dtype, hipStream_t s) {
  const long long kp_rows = k / 2;
  const long long total = kp_rows * (n / 8);
  if (total == 0) return;
  dim3 grid((unsigned)elementwise_grid((total + 255) / 256));
  const int gshift = group_shift(group_size);
  if (dtype == kBF16)
    hipLaunchKernelGGL((dequant_int4_kernel<true>), grid, dim3(256), 0, s,
                       (const signed char*)qw, scale, out, kp_rows,
                       (long long)n, gshift);
  else
    hipLaunchKernelGGL((dequant_int4_kernel<false>), grid, dim3(256), 0, s,
                       (const signed char*)qw, scale, out, kp_rows,
                       (long long)n, gshift);
}

}  // namespace pa
