// Shared by the decode W-streamers (decode_gemm.hip, decode_gemm_mx.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pa {

// Launches decode_gemm_reduce_kernel (decode_gemm.hip): y[m][n] bf16 = (sum
// over `splits` of workspace[s][mt][n] fp32) * qinv (* chscale[n]) (+ bias[n]).
void decode_gemm_launch_reduce(const float* workspace, const float* chscale,
                               float qinv, const void* bias, void* y,
                               int64_t m, int64_t n, int mt, int splits,
                               hipStream_t s);

}  // namespace pa
