// LayerNorm / RMSNorm forward+backward for gfx950.
//
// Design (MI355X): these are HBM-bandwidth-bound at D=4096..8192; the
// kernels do one vectorized pass per row (256-thread block per row,
// 16B/lane loads), fp32 accumulation, wave64 shuffle + 4-slot LDS block
// reduction.  Up to D = 8192 the residual add + LayerNorm forward and the
// whole LayerNorm backward (dx, residual gradient, dgamma/dbeta) are
// register-resident single passes (add_ln_fwd_kernel, ln_bwd_fused_kernel);
// wider rows and RMSNorm use the per-row dx kernel plus a column-parallel
// dgamma/dbeta kernel writing per-chunk partials for a reduce kernel.
//
// Reference behavior parity: paddle/phi/kernels/gpu/layer_norm_kernel.cu
// (LayerNormFwdWithWelford) and rms_norm_kernel.cu (cuApplyRMSNorm) --
// re-derived, not ported.  LayerNorm's variance uses shifted single-pass
// moments (see ln_fwd_kernel), not Welford merging; both are robust to a
// row mean far from zero.
#include "row_io.h"

namespace pa {

// ---------------------------------------------------------------------------
// Pinned row arithmetic.  Each LayerNorm pass exists twice -- the generic
// kernel that re-reads the row and the register-resident fused kernel -- and
// the two must agree bit for bit (tests/test_fused_passes_gpu.py).  Under
// -ffast-math the compiler otherwise picks the summation tree and the fma
// contractions per kernel, so the shared steps live in these helpers:
// reassociation off, fused multiply-adds spelled out, and pin() where a
// product must be rounded before its consumer.
// ---------------------------------------------------------------------------
// v, materialised in a VGPR: nothing contracts or reassociates through it
__device__ __forceinline__ float pin(float v) {
  asm("" : "+v"(v));
  return v;
}

// Value as stored in T and read back.  bf16: the round trip.  fp32: pinned,
// so that a following add is not contracted with the producing multiply.
template <int DT>
__device__ __forceinline__ float round_t(float v) {
  if (DT == kBF16) return bf2f(f2bf(v));
  return pin(v);
}

// K of the shifted moments: mean of the row's first 8 elements, summed left
// to right.
__device__ __forceinline__ float row_shift8(const float* f0) {
#pragma clang fp reassociate(off)
  float s = ((((((f0[0] + f0[1]) + f0[2]) + f0[3]) + f0[4]) + f0[5]) + f0[6]) + f0[7];
  return s * 0.125f;
}

// forward moments of one element: sum += f, sumc += f-K, sumsq += (f-K)^2
// with the square rounded before the add
__device__ __forceinline__ void ln_moments(float f, float shift, float& sum,
                                           float& sumc, float& sumsq) {
  // reassociate(off): -ffast-math may otherwise fold the eight "- shift"
  // into one "- 8*shift" after summing the raw values
#pragma clang fp reassociate(off)
  float c = f - shift;
  sum += f;
  sumc += c;
  sumsq += pin(c * c);
}

// y = (f - mu) * rstd * w + b, evaluated as fma(w * rstd, f - mu, b)
__device__ __forceinline__ float ln_y(float f, float mu, float rstd, float w, float b) {
#pragma clang fp reassociate(off)
  return __builtin_fmaf(pin(w * rstd), f - mu, b);
}

__device__ __forceinline__ float ln_xhat(float x, float mu, float rs) {
  return pin((x - mu) * rs);
}

// backward row sums of one element: s1 += g*xhat, s2 += g, g = dy*w rounded
__device__ __forceinline__ void ln_bwd_sums(float gy, float w, float xh,
                                            float& s1, float& s2) {
#pragma clang fp reassociate(off)
  float g = pin(gy * w);
  s1 = __builtin_fmaf(g, xh, s1);
  s2 += g;
}

// dx = rs * (g - c2 - xhat * c1), c1 = mean(g*xhat), c2 = mean(g)
__device__ __forceinline__ float ln_bwd_dx1(float gy, float w, float xh, float c1,
                                            float c2, float rs) {
#pragma clang fp reassociate(off)
  float g = pin(gy * w);
  float a = pin(g - c2);
  return rs * __builtin_fmaf(-xh, c1, a);
}

// ---------------------------------------------------------------------------
// LayerNorm forward: one 256-thread block per row.
// ---------------------------------------------------------------------------
template <int DT>
__global__ void ln_fwd_kernel(const void* __restrict__ x, const void* __restrict__ w,
                              const void* __restrict__ b, void* __restrict__ y,
                              float* __restrict__ mean_out, float* __restrict__ rstd_out,
                              int64_t n, int64_t d, float eps) {
  __shared__ float red[12];
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const int64_t base = row * d;
    // Shifted moments: the variance comes from sum(x-K) and sum((x-K)^2).
    // E[x^2] - mu^2 on the raw values cancels in fp32 once |mu| >> sigma
    // (var clamps to 0 near mu = 3000*sigma); after the shift the same
    // identity only cancels against (mu - K)^2.  K is the mean of the row's
    // first 8 elements (one broadcast load per row, d % 8 == 0), so that one
    // outlier in column 0 moves K by an eighth of its size only.  A row whose
    // first 8 elements all sit far from the rest (|K - mu| >> sigma) still
    // loses log2((K-mu)^2/var) bits of the variance.
    // The mean itself is the plain sum / d: K + mean(x-K) would round at
    // ulp(K), which is coarse when |mu| << |K|.
    float shift;
    {
      float f0[8];
      VIO<DT>::load8(x, base, f0);
      shift = row_shift8(f0);
    }
    float sum = 0.f, sumc = 0.f, sumsq = 0.f;
    for (int64_t i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
      float f[8];
      VIO<DT>::load8(x, base + i, f);
#pragma unroll
      for (int k = 0; k < 8; ++k) ln_moments(f[k], shift, sum, sumc, sumsq);
    }
    float ts = block_reduce_256(sum, SumOp(), red, 0.f);
    float tsc = block_reduce_256(sumc, SumOp(), red + 4, 0.f);
    float tss = block_reduce_256(sumsq, SumOp(), red + 8, 0.f);
    float mu = ts / d;
    float dmu = tsc / d;  // mean of the shifted row
    float var = fmaxf(tss / d - dmu * dmu, 0.f);
    float rstd = rsqrtf(var + eps);
    if (threadIdx.x == 0) { mean_out[row] = mu; rstd_out[row] = rstd; }
    for (int64_t i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
      float f[8], wf[8], bf[8];
      VIO<DT>::load8(x, base + i, f);
      VIO<DT>::load8(w, i, wf);
      if (b) VIO<DT>::load8(b, i, bf);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        f[k] = ln_y(f[k], mu, rstd, wf[k], b ? bf[k] : 0.f);
      VIO<DT>::store8(y, base + i, f);
    }
    __syncthreads();
  }
}

// dx = rstd * (g - mean(g) - xhat * mean(g*xhat)),  g = dy*w
template <int DT>
__global__ void ln_bwd_dx_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                 const void* __restrict__ w, const float* __restrict__ mean,
                                 const float* __restrict__ rstd, void* __restrict__ dx,
                                 int64_t n, int64_t d) {
  __shared__ float red[8];
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const int64_t base = row * d;
    const float mu = mean[row], rs = rstd[row];
    float s1 = 0.f, s2 = 0.f;  // sum(g*xhat), sum(g)
    for (int64_t i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
      float gy[8], xf[8], wf[8];
      VIO<DT>::load8(dy, base + i, gy);
      VIO<DT>::load8(x, base + i, xf);
      VIO<DT>::load8(w, i, wf);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        ln_bwd_sums(gy[k], wf[k], ln_xhat(xf[k], mu, rs), s1, s2);
    }
    float t1 = block_reduce_256(s1, SumOp(), red, 0.f);
    __syncthreads();
    float t2 = block_reduce_256(s2, SumOp(), red + 4, 0.f);
    const float inv_d = 1.f / d;
    const float c1 = pin(t1 * inv_d), c2 = pin(t2 * inv_d);
    for (int64_t i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
      float gy[8], xf[8], wf[8];
      VIO<DT>::load8(dy, base + i, gy);
      VIO<DT>::load8(x, base + i, xf);
      VIO<DT>::load8(w, i, wf);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        gy[k] = ln_bwd_dx1(gy[k], wf[k], ln_xhat(xf[k], mu, rs), c1, c2, rs);
      VIO<DT>::store8(dx, base + i, gy);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Column reductions [n, d] -> fp32 [d] of the two-kernel backward: LayerNorm
// dw/db (2 planes) and RMSNorm dw (1 plane).  A thread owns an 8-wide column
// strip (16 B loads, d % 8 == 0) and walks the rows of its chunk (blockIdx.y)
// in row order.  The chunk's sums go to ws[chunk][NOUT][d] with plain stores
// and ws_reduce_kernel adds the chunks in a fixed order.  (One fp32 atomic
// per (column, chunk) instead serializes ~chunks adds per column at one L2
// bank: measured 3x over the HBM bound at n = 24k, d = 4k.)
// ---------------------------------------------------------------------------
// one element's terms: dy*xhat and dy | dy*x*rstd.  The products are
// associated as written, fma(dy*rstd, x - mu, s0) and fma(x*rstd, dy, s0):
// left to -ffast-math the association changes with the surrounding code.
template <bool RMS>
__device__ __forceinline__ void col_term(float g, float x, float mu, float rs,
                                         float& s0, float& s1) {
#pragma clang fp reassociate(off)
  if (RMS) {
    s0 = __builtin_fmaf(x * rs, g, s0);
  } else {
    s0 = __builtin_fmaf(g * rs, x - mu, s0);
    s1 += g;
  }
}

template <int DT, bool RMS>
__global__ void col_partial_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                   float* __restrict__ ws, int64_t n, int64_t d) {
  constexpr int NOUT = RMS ? 1 : 2;
  int64_t c0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (c0 >= d) return;
  int64_t rows_per = (n + gridDim.y - 1) / gridDim.y;
  int64_t r0 = (int64_t)blockIdx.y * rows_per;
  int64_t r1 = min(n, r0 + rows_per);
  float s0[8] = {0.f}, s1[8] = {0.f};
  for (int64_t r = r0; r < r1; ++r) {
    float g[8], xf[8];
    VIO<DT>::load8(dy, r * d + c0, g);
    VIO<DT>::load8(x, r * d + c0, xf);
    float mu = RMS ? 0.f : mean[r], rs = rstd[r];
#pragma unroll
    for (int k = 0; k < 8; ++k) col_term<RMS>(g[k], xf[k], mu, rs, s0[k], s1[k]);
  }
  float* wrow = ws + (int64_t)blockIdx.y * NOUT * d;
  VIO<kF32>::store8(wrow, c0, s0);
  if (NOUT == 2) VIO<kF32>::store8(wrow, d + c0, s1);
}

// ---------------------------------------------------------------------------
// Fused residual add + LayerNorm forward: h = x + residual (stored in T),
// y = LN(h) from the stored h.  Thread t owns the 8-wide column strips
// t*8 + j*2048, j < NS (d <= NS*2048), and keeps its slice of h in
// registers, so h is written once and never read back.  Sums run in the
// order of ln_fwd_kernel: y / mean / rstd are bit-equal to
// dropout_add_fwd(p=0) followed by ln_fwd_kernel.
// ---------------------------------------------------------------------------
template <int DT, int NS>
__global__ __launch_bounds__(256) void add_ln_fwd_kernel(
    const void* __restrict__ x, const void* __restrict__ res,
    const void* __restrict__ w, const void* __restrict__ b,
    void* __restrict__ h, void* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int64_t n, int64_t d, float eps) {
  __shared__ float red[12];
  const int64_t c0 = threadIdx.x * 8;
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const int64_t base = row * d;
    float shift;
    {
      float f0[8], r0[8];
      VIO<DT>::load8(x, base, f0);
      VIO<DT>::load8(res, base, r0);
#pragma unroll
      for (int k = 0; k < 8; ++k) f0[k] = round_t<DT>(f0[k] + r0[k]);
      shift = row_shift8(f0);
    }
    float hf[NS][8];
    float sum = 0.f, sumc = 0.f, sumsq = 0.f;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int64_t c = c0 + (int64_t)j * 2048;
      if (c < d) {
        float rf[8];
        VIO<DT>::load8(x, base + c, hf[j]);
        VIO<DT>::load8(res, base + c, rf);
#pragma unroll
        for (int k = 0; k < 8; ++k) hf[j][k] = round_t<DT>(hf[j][k] + rf[k]);
        VIO<DT>::store8(h, base + c, hf[j]);
#pragma unroll
        for (int k = 0; k < 8; ++k) ln_moments(hf[j][k], shift, sum, sumc, sumsq);
      }
    }
    float ts = block_reduce_256(sum, SumOp(), red, 0.f);
    float tsc = block_reduce_256(sumc, SumOp(), red + 4, 0.f);
    float tss = block_reduce_256(sumsq, SumOp(), red + 8, 0.f);
    float mu = ts / d;
    float dmu = tsc / d;
    float var = fmaxf(tss / d - dmu * dmu, 0.f);
    float rstd = rsqrtf(var + eps);
    if (threadIdx.x == 0) { mean_out[row] = mu; rstd_out[row] = rstd; }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int64_t c = c0 + (int64_t)j * 2048;
      if (c < d) {
        float wf[8], bf[8], f[8];
        VIO<DT>::load8(w, c, wf);
        if (b) VIO<DT>::load8(b, c, bf);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          f[k] = ln_y(hf[j][k], mu, rstd, wf[k], b ? bf[k] : 0.f);
        VIO<DT>::store8(y, base + c, f);
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// One-pass LayerNorm backward: dx (+ optional residual gradient) and the
// dw/db partials from a single read of dy and x.  Column ownership as in
// add_ln_fwd_kernel; the thread keeps dy and xhat of the row in registers
// between the row sums and the dx pass, and accumulates dy*xhat / dy of its
// own columns over all rows of the block.  The block's partials go to
// ws[blockIdx.x][2][d] with plain stores; ws_reduce_kernel sums them.
// The row sums s1 / s2 run in the order of ln_bwd_dx_kernel.
// dres: dx = round_T(round_T(LN term) + dres), i.e. what ln_bwd_dx_kernel
// followed by a tensor add in T gives.
// ---------------------------------------------------------------------------
template <int DT, int NS, bool HAS_DRES>
__global__ __launch_bounds__(256) void ln_bwd_fused_kernel(
    const void* __restrict__ dy, const void* __restrict__ x,
    const void* __restrict__ w, const float* __restrict__ mean,
    const float* __restrict__ rstd, const void* __restrict__ dres,
    void* __restrict__ dx, float* __restrict__ ws, int64_t n, int64_t d) {
  __shared__ float red[8];
  const int64_t c0 = threadIdx.x * 8;
  float wf[NS][8], aw[NS][8], ab[NS][8];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int64_t c = c0 + (int64_t)j * 2048;
#pragma unroll
    for (int k = 0; k < 8; ++k) { wf[j][k] = 0.f; aw[j][k] = 0.f; ab[j][k] = 0.f; }
    if (c < d) VIO<DT>::load8(w, c, wf[j]);
  }
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const int64_t base = row * d;
    const float mu = mean[row], rs = rstd[row];
    float gy[NS][8], xh[NS][8];
    float s1 = 0.f, s2 = 0.f;  // sum(g*xhat), sum(g)
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int64_t c = c0 + (int64_t)j * 2048;
      if (c < d) {
        VIO<DT>::load8(dy, base + c, gy[j]);
        VIO<DT>::load8(x, base + c, xh[j]);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          xh[j][k] = ln_xhat(xh[j][k], mu, rs);
          ln_bwd_sums(gy[j][k], wf[j][k], xh[j][k], s1, s2);
        }
      }
    }
    float t1 = block_reduce_256(s1, SumOp(), red, 0.f);
    __syncthreads();
    float t2 = block_reduce_256(s2, SumOp(), red + 4, 0.f);
    const float inv_d = 1.f / d;
    const float c1 = pin(t1 * inv_d), c2 = pin(t2 * inv_d);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int64_t c = c0 + (int64_t)j * 2048;
      if (c < d) {
        float o[8], rf[8];
        if (HAS_DRES) VIO<DT>::load8(dres, base + c, rf);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          o[k] = ln_bwd_dx1(gy[j][k], wf[j][k], xh[j][k], c1, c2, rs);
          if (HAS_DRES) o[k] = round_t<DT>(o[k]) + rf[k];
          aw[j][k] += gy[j][k] * xh[j][k];
          ab[j][k] += gy[j][k];
        }
        VIO<DT>::store8(dx, base + c, o);
      }
    }
    __syncthreads();
  }
  float* wrow = ws + (int64_t)blockIdx.x * 2 * d;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int64_t c = c0 + (int64_t)j * 2048;
    if (c < d) {
      VIO<kF32>::store8(wrow, c, aw[j]);
      VIO<kF32>::store8(wrow, d + c, ab[j]);
    }
  }
}

// Sum partials ws[parts][nout][d] over parts -> out[o][d], o = blockIdx.y.
// 1024 threads: wave v adds parts v, v+16, ... for 64 columns (256 B per
// load), the 16 wave sums meet in LDS and are added in wave order, so the
// result does not depend on scheduling.  d/64 x nout blocks keep every CU
// busy where a serial walk on d/256 blocks would not.
__global__ __launch_bounds__(1024) void ws_reduce_kernel(
    const float* __restrict__ ws, float* __restrict__ out0,
    float* __restrict__ out1, int parts, int nout, int64_t d) {
  __shared__ float lds[16][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const int o = blockIdx.y;
  float acc = 0.f;
  if (c < d)
    for (int p = wv; p < parts; p += 16)
      acc += ws[((int64_t)p * nout + o) * d + c];
  lds[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && c < d) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += lds[i][lane];
    (o == 0 ? out0 : out1)[c] = s;
  }
}

// ---------------------------------------------------------------------------
// RMSNorm (optionally fused residual-add: xr = x + residual; y = rms(xr)*w,
// res_out = xr) -- matches fused_rms_norm semantics.
// ---------------------------------------------------------------------------
template <int DT, bool HAS_RES>
__global__ void rms_fwd_kernel(const void* __restrict__ x, const void* __restrict__ res,
                               const void* __restrict__ w, void* __restrict__ y,
                               void* __restrict__ res_out, float* __restrict__ rstd_out,
                               int64_t n, int64_t d, float eps) {
  __shared__ float red[4];
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const int64_t base = row * d;
    float sumsq = 0.f;
    for (int64_t i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
      float f[8];
      VIO<DT>::load8(x, base + i, f);
      if (HAS_RES) {
        float r[8];
        VIO<DT>::load8(res, base + i, r);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] += r[k];
        VIO<DT>::store8(res_out, base + i, f);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) sumsq += f[k] * f[k];
    }
    // no barrier for res_out: each thread reads back only what it stored itself
    float tss = block_reduce_256(sumsq, SumOp(), red, 0.f);
    float rstd = rsqrtf(tss / d + eps);
    if (threadIdx.x == 0) rstd_out[row] = rstd;
    const void* src = HAS_RES ? res_out : x;
    for (int64_t i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
      float f[8], wf[8];
      VIO<DT>::load8(src, base + i, f);
      VIO<DT>::load8(w, i, wf);
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = f[k] * rstd * wf[k];
      VIO<DT>::store8(y, base + i, f);
    }
    __syncthreads();
  }
}

// dx = rstd*(g - xhat * mean(g*xhat)),  g = dy*w, xhat = x*rstd
template <int DT>
__global__ void rms_bwd_dx_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                  const void* __restrict__ w, const float* __restrict__ rstd,
                                  void* __restrict__ dx, int64_t n, int64_t d) {
  __shared__ float red[4];
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const int64_t base = row * d;
    const float rs = rstd[row];
    float s1 = 0.f;
    for (int64_t i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
      float gy[8], xf[8], wf[8];
      VIO<DT>::load8(dy, base + i, gy);
      VIO<DT>::load8(x, base + i, xf);
      VIO<DT>::load8(w, i, wf);
#pragma unroll
      for (int k = 0; k < 8; ++k) s1 += gy[k] * wf[k] * xf[k] * rs;
    }
    float t1 = block_reduce_256(s1, SumOp(), red, 0.f);
    const float c = t1 / d;
    for (int64_t i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
      float gy[8], xf[8], wf[8];
      VIO<DT>::load8(dy, base + i, gy);
      VIO<DT>::load8(x, base + i, xf);
      VIO<DT>::load8(w, i, wf);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        gy[k] = rs * (gy[k] * wf[k] - xf[k] * rs * c);
      VIO<DT>::store8(dx, base + i, gy);
    }
    __syncthreads();
  }
}

// -------- host launchers ----------------------------------------------------
static int norm_grid(int64_t n) {
  int64_t cap = 256 * 8;
  return (int)(n < cap ? n : cap);
}

// strip count of the register-resident kernels, 1..4 for d <= 8192, as a
// std::integral_constant
template <class F>
static void by_strips(int64_t d, F&& f) {
  switch (cdiv((int)d, 2048)) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

void layer_norm_fwd(const void* x, const void* w, const void* b, void* y,
                    float* mean, float* rstd, int64_t n, int64_t d, float eps,
                    int dtype, hipStream_t s) {
  by_dtype(dtype, [&](auto DT) {
    hipLaunchKernelGGL((ln_fwd_kernel<DT()>), dim3(norm_grid(n)), dim3(256), 0, s,
                       x, w, b, y, mean, rstd, n, d, eps);
  });
}

void layer_norm_bwd_dx(const void* dy, const void* x, const void* w,
                       const float* mean, const float* rstd, void* dx,
                       int64_t n, int64_t d, int dtype, hipStream_t s) {
  by_dtype(dtype, [&](auto DT) {
    hipLaunchKernelGGL((ln_bwd_dx_kernel<DT()>), dim3(norm_grid(n)), dim3(256), 0, s,
                       dy, x, w, mean, rstd, dx, n, d);
  });
}

bool ln_fused_ok(int64_t d) { return d % 8 == 0 && d <= kLnFusedMaxD; }

int ln_bwd_fused_grid(int64_t n, int cap) {
  if (cap <= 0) cap = kLnBwdGridCap;
  return (int)hmin<int64_t>(n, cap);
}

void ws_reduce(const float* ws, float* out0, float* out1, int parts, int nout,
               int64_t d, hipStream_t s) {
  dim3 grid((unsigned)((d + 63) / 64), out1 ? 2 : 1);
  hipLaunchKernelGGL(ws_reduce_kernel, grid, dim3(1024), 0, s, ws, out0, out1,
                     parts, nout, d);
}

// row chunks of the column reductions (and of colsum): keep >= 1024
// workgroups in flight (256 CUs / 8 XCDs want oversubscription), at least 32
// rows per chunk
int col_chunks(int64_t n, int64_t d) {
  int xblocks = cdiv((int)d, 256 * 8);
  return (int)hmin<int64_t>(hmax<int64_t>(1, n / 32),
                            hmax<int64_t>(1, 2048 / xblocks));
}

template <bool RMS>
static void col_reduce(const void* dy, const void* x, const float* mean,
                       const float* rstd, float* dw, float* db, float* ws,
                       int64_t n, int64_t d, int dtype, hipStream_t s) {
  const int chunks = col_chunks(n, d);
  dim3 grid((unsigned)cdiv((int)d, 256 * 8), chunks);
  by_dtype(dtype, [&](auto DT) {
    hipLaunchKernelGGL((col_partial_kernel<DT(), RMS>), grid, dim3(256), 0, s,
                       dy, x, mean, rstd, ws, n, d);
  });
  ws_reduce(ws, dw, db, chunks, RMS ? 1 : 2, d, s);
}

void layer_norm_bwd_dwdb(const void* dy, const void* x, const float* mean,
                         const float* rstd, float* dw, float* db, float* ws,
                         int64_t n, int64_t d, int dtype, hipStream_t s) {
  col_reduce<false>(dy, x, mean, rstd, dw, db, ws, n, d, dtype, s);
}

void rms_norm_bwd_dw(const void* dy, const void* x, const float* rstd,
                     float* dw, float* ws, int64_t n, int64_t d, int dtype,
                     hipStream_t s) {
  col_reduce<true>(dy, x, nullptr, rstd, dw, nullptr, ws, n, d, dtype, s);
}

void add_layer_norm_fwd(const void* x, const void* residual, const void* w,
                        const void* b, void* h, void* y, float* mean,
                        float* rstd, int64_t n, int64_t d, float eps, int dtype,
                        hipStream_t s) {
  by_dtype(dtype, [&](auto DT) {
    by_strips(d, [&](auto NS) {
      hipLaunchKernelGGL((add_ln_fwd_kernel<DT(), NS()>), dim3(norm_grid(n)),
                         dim3(256), 0, s, x, residual, w, b, h, y, mean, rstd, n, d, eps);
    });
  });
}

void layer_norm_bwd_fused(const void* dy, const void* x, const void* w,
                          const float* mean, const float* rstd,
                          const void* dres, void* dx, float* dw, float* db,
                          float* ws, int grid, int64_t n, int64_t d, int dtype,
                          hipStream_t s) {
  by_dtype(dtype, [&](auto DT) {
    by_strips(d, [&](auto NS) {
      by_flag(dres != nullptr, [&](auto HAS_DRES) {
        hipLaunchKernelGGL((ln_bwd_fused_kernel<DT(), NS(), HAS_DRES()>), dim3(grid),
                           dim3(256), 0, s, dy, x, w, mean, rstd, dres, dx, ws, n, d);
      });
    });
  });
  ws_reduce(ws, dw, db, grid, 2, d, s);
}

void rms_norm_fwd(const void* x, const void* residual, const void* w, void* y,
                  void* res_out, float* rstd, int64_t n, int64_t d, float eps,
                  int dtype, hipStream_t s) {
  by_dtype(dtype, [&](auto DT) {
    by_flag(residual != nullptr, [&](auto HAS_RES) {
      hipLaunchKernelGGL((rms_fwd_kernel<DT(), HAS_RES()>), dim3(norm_grid(n)),
                         dim3(256), 0, s, x, residual, w, y, res_out, rstd, n, d, eps);
    });
  });
}

void rms_norm_bwd_dx(const void* dy, const void* x, const void* w,
                     const float* rstd, void* dx, int64_t n, int64_t d,
                     int dtype, hipStream_t s) {
  by_dtype(dtype, [&](auto DT) {
    hipLaunchKernelGGL((rms_bwd_dx_kernel<DT()>), dim3(norm_grid(n)), dim3(256), 0, s,
                       dy, x, w, rstd, dx, n, d);
  });
}

}  // namespace pa
