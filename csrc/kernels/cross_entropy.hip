// Fused softmax + cross-entropy (hard labels) for gfx950.
//
// One 256-thread block per row, online (max,sum) accumulation in a single
// pass over V (vocab ~50k: 2 passes over HBM total for fwd incl. store of
// nothing -- we keep only lse + loss, grads recompute exp in bwd).
//
// Reference behavior parity: paddle/phi/kernels/gpu/cross_entropy_kernel.cu
// (VectorizedSoftmaxForward / WarpSoftmaxForward) -- re-derived for wave64.
#include "row_io.h"

namespace pa {

// Running maximum of a lane that has seen nothing yet.  It is the largest
// finite negative float, not -inf: a -inf logit (a banned token) that arrives
// while the maximum is still "empty" then gives x - m = -inf and adds
// exp(-inf) = 0, where -inf - -inf would be NaN.  Testing for infinity
// instead does not work in this tree: it is built with -ffast-math, which
// lets the compiler fold such a test away (bit-pattern compares included).
#define LSE_EMPTY (-3.402823466e+38f)

// one online-softmax step
__device__ __forceinline__ void lse_step(float& m, float& l, float x) {
  if (x > m) { l *= __expf(m - x); m = x; }
  l += __expf(x - m);
}

// merge two (max, sumexp) pairs; m - mn is <= 0, finite or -inf, never NaN
__device__ __forceinline__ void lse_merge(float& m, float& l, float m2, float l2) {
  float mn = fmaxf(m, m2);
  float a = (m == mn) ? l : l * __expf(m - mn);
  float b = (m2 == mn) ? l2 : l2 * __expf(m2 - mn);
  l = a + b;
  m = mn;
}

template <int DT>
__global__ void ce_fwd_kernel(const void* __restrict__ logits,
                              const int64_t* __restrict__ labels,
                              float* __restrict__ loss, float* __restrict__ lse_out,
                              int64_t n, int64_t v, int64_t ignore_index) {
  __shared__ float red_m[4], red_l[4];
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const int64_t base = row * v;
    float m = LSE_EMPTY, l = 0.f;
    int64_t i = threadIdx.x * 8;
    const int64_t v8 = v & ~7LL;
    for (; i < v8; i += blockDim.x * 8) {
      float f[8];
      VIO<DT>::load8(logits, base + i, f);
#pragma unroll
      for (int k = 0; k < 8; ++k) lse_step(m, l, f[k]);
    }
    // tail
    for (int64_t j = v8 + threadIdx.x; j < v; j += blockDim.x) {
      lse_step(m, l, VIO<DT>::load1(logits, base + j));
    }
    // wave reduce
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      float m2 = __shfl_xor(m, off, WAVE);
      float l2 = __shfl_xor(l, off, WAVE);
      lse_merge(m, l, m2, l2);
    }
    int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red_m[wid] = m; red_l[wid] = l; }
    __syncthreads();
    m = red_m[0]; l = red_l[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) lse_merge(m, l, red_m[k], red_l[k]);
    float lse = m + __logf(l);
    if (threadIdx.x == 0) {
      int64_t lab = labels[row];
      lse_out[row] = lse;
      // a label outside [0, v) is never dereferenced: like ignore_index it
      // contributes zero loss (and zero gradient in ce_bwd_kernel)
      if (lab == ignore_index || lab < 0 || lab >= v) {
        loss[row] = 0.f;
      } else {
        float xl = VIO<DT>::load1(logits, base + lab);
        loss[row] = lse - xl;
      }
    }
    __syncthreads();
  }
}

template <int DT>
__global__ void ce_bwd_kernel(const float* __restrict__ dloss,
                              const void* __restrict__ logits,
                              const int64_t* __restrict__ labels,
                              const float* __restrict__ lse, void* __restrict__ dlogits,
                              int64_t n, int64_t v, int64_t ignore_index) {
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const int64_t base = row * v;
    const int64_t lab = labels[row];
    const float g = (lab == ignore_index || lab < 0 || lab >= v) ? 0.f : dloss[row];
    const float ls = lse[row];
    const int64_t v8 = v & ~7LL;
    int64_t i = threadIdx.x * 8;
    for (; i < v8; i += blockDim.x * 8) {
      float f[8];
      VIO<DT>::load8(logits, base + i, f);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float p = __expf(f[k] - ls);
        f[k] = g * (p - ((i + k) == lab ? 1.f : 0.f));
      }
      VIO<DT>::store8(dlogits, base + i, f);
    }
    for (int64_t j = v8 + threadIdx.x; j < v; j += blockDim.x) {
      float p = __expf(VIO<DT>::load1(logits, base + j) - ls);
      VIO<DT>::store1(dlogits, base + j, g * (p - (j == lab ? 1.f : 0.f)));
    }
  }
}

void softmax_ce_fwd(const void* logits, const int64_t* labels, float* loss,
                    float* lse, int64_t n, int64_t v, int64_t ignore_index,
                    int dtype, hipStream_t s) {
  int grid = (int)(n < 2048 ? n : 2048);
  by_dtype(dtype, [&](auto DT) {
    hipLaunchKernelGGL((ce_fwd_kernel<DT()>), dim3(grid), dim3(256), 0, s,
                       logits, labels, loss, lse, n, v, ignore_index);
  });
}

void softmax_ce_bwd(const float* dloss, const void* logits,
                    const int64_t* labels, const float* lse, void* dlogits,
                    int64_t n, int64_t v, int64_t ignore_index, int dtype,
                    hipStream_t s) {
  int grid = (int)(n < 2048 ? n : 2048);
  by_dtype(dtype, [&](auto DT) {
    hipLaunchKernelGGL((ce_bwd_kernel<DT()>), dim3(grid), dim3(256), 0, s,
                       dloss, logits, labels, lse, dlogits, n, v, ignore_index);
  });
}

}  // namespace pa
