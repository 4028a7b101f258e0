// MoE row movers for gfx950: dispatch (tokens -> capacity slots), combine
// (slots -> tokens, weighted sum over k) and the combine backward, all over
// the slot maps of moe_route (moe.hip).  docs/KERNELS.md "MoE dispatch /
// combine".
//
// One layout for the three kernels.  A row is cut into 16-byte pieces; a
// group of `lpr` = 2^lg lanes (the smallest power of two covering the pieces,
// at most one wave) owns one output row and strides over its pieces, so a
// 256-thread block carries 256 / lpr rows: 4 rows at h >= 512 bf16, 256 rows
// at h = 8.  Lanes of a group read and write consecutive 16-byte pieces; the
// map entry of a row is one broadcast load.
//
// Every output row is written exactly once by plain stores: dispatch and the
// combine backward walk the slots (an empty slot stores zeros), combine walks
// the tokens (a token with every choice dropped stores zeros).  No memset, no
// atomics, no host read.  A map entry outside its range counts as empty /
// dropped and is never used as an index.
#include "row_io.h"

namespace pa {

namespace {

struct RowPlan { int lg; unsigned grid; };

// pieces: 16-byte (dispatch) or 8-element (combine) pieces per row
RowPlan row_plan(int64_t rows, int64_t pieces) {
  RowPlan p{0, 0};
  while ((1 << p.lg) < pieces && p.lg < 6) ++p.lg;
  const int64_t rpb = 256 >> p.lg;
  p.grid = (unsigned)((rows + rpb - 1) / rpb);
  return p;
}

// out[s] = x[src_of[s] / K] or zeros; rows as raw 16-byte pieces, so the copy
// is bit-exact for every dtype.  pieces = row bytes / 16.
__global__ __launch_bounds__(256) void moe_dispatch_kernel(
    const intx4* __restrict__ x, const int* __restrict__ src_of,
    intx4* __restrict__ out, int S, int TK, int K, int pieces, int lg) {
  const int lpr = 1 << lg;
  const int c = threadIdx.x & (lpr - 1);
  const int64_t s = (int64_t)blockIdx.x * (256 >> lg) + (threadIdx.x >> lg);
  if (s >= S) return;
  const int src = src_of[s];
  const bool ok = (unsigned)src < (unsigned)TK;
  const intx4* xr = x + (int64_t)(ok ? src / K : 0) * pieces;
  intx4* orow = out + s * pieces;
  for (int p = c; p < pieces; p += lpr) {
    intx4 v = {0, 0, 0, 0};
    if (ok) v = xr[p];
    orow[p] = v;
  }
}

// out[t] = sum_kk w[t, kk] * y[slot_of[t, kk]] over the kept kk, fp32
// accumulation in kk order, one rounding.  WEIGHTED = false: weight 1 (the
// backward of dispatch).
template <int DT, bool WEIGHTED>
__global__ __launch_bounds__(256) void moe_combine_kernel(
    const void* __restrict__ y, const float* __restrict__ w,
    const int* __restrict__ slot_of, void* __restrict__ out, int T, int K,
    int S, int h, int lg) {
  const int lpr = 1 << lg;
  const int c = threadIdx.x & (lpr - 1);
  const int64_t t = (int64_t)blockIdx.x * (256 >> lg) + (threadIdx.x >> lg);
  if (t >= T) return;
  const int* sl = slot_of + t * K;
  const float* wt = WEIGHTED ? w + t * K : nullptr;
  const int pieces = h >> 3;
  for (int p = c; p < pieces; p += lpr) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < K; ++kk) {
      const int slot = sl[kk];
      if ((unsigned)slot >= (unsigned)S) continue;
      float v[8];
      VIO<DT>::load8(y, (int64_t)slot * h + p * 8, v);
      const float g = WEIGHTED ? wt[kk] : 1.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += g * v[i];
    }
    VIO<DT>::store8(out, t * h + p * 8, acc);
  }
}

// Slot s with src = src_of[s] in range, t = src / K:
//   dy[s] = w[src] * dout[t]              (one rounding)
//   dw[src] = sum_h y[s, h] * dout[t, h]  (fp32)
// else dy[s] = 0 and dw is not touched (the binding hands it over zeroed).
// The dot product runs over a lane's pieces in order, then over the lpr lanes
// of the row by an xor butterfly: the same order on every call.
template <int DT>
__global__ __launch_bounds__(256) void moe_combine_bwd_kernel(
    const void* __restrict__ y, const void* __restrict__ dout,
    const float* __restrict__ w, const int* __restrict__ src_of,
    void* __restrict__ dy, float* __restrict__ dw, int S, int TK, int K, int h,
    int lg) {
  const int lpr = 1 << lg;
  const int c = threadIdx.x & (lpr - 1);
  const int64_t s = (int64_t)blockIdx.x * (256 >> lg) + (threadIdx.x >> lg);
  const bool row = s < S;
  const int src = row ? src_of[s] : -1;
  const bool ok = (unsigned)src < (unsigned)TK;
  const int64_t t = ok ? src / K : 0;
  const float g = ok ? w[src] : 0.f;
  const int pieces = h >> 3;
  float dot = 0.f;
  if (row) {
    for (int p = c; p < pieces; p += lpr) {
      float d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (ok) {
        float v[8];
        VIO<DT>::load8(dout, t * h + p * 8, d);
        VIO<DT>::load8(y, s * h + p * 8, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          dot += v[i] * d[i];
          d[i] *= g;
        }
      }
      VIO<DT>::store8(dy, s * h + p * 8, d);
    }
  }
  // every lane of the wave arrives here: groups are lpr-aligned inside it
  for (int off = lpr >> 1; off > 0; off >>= 1) dot += __shfl_xor(dot, off, WAVE);
  if (ok && c == 0) dw[src] = dot;
}

}  // namespace

void moe_dispatch(const MoePermuteArgs& a, hipStream_t s) {
  const int64_t pieces = (int64_t)a.h * (a.dtype == kBF16 ? 2 : 4) / 16;
  const RowPlan p = row_plan(a.slots, pieces);
  hipLaunchKernelGGL(moe_dispatch_kernel, dim3(p.grid), dim3(256), 0, s,
                     (const intx4*)a.x, a.src_of, (intx4*)a.out, a.slots,
                     a.t * a.k, a.k, (int)pieces, p.lg);
}

void moe_combine(const MoePermuteArgs& a, hipStream_t s) {
  const RowPlan p = row_plan(a.t, a.h / 8);
  by_dtype(a.dtype, [&](auto DT) {
    by_flag(a.w != nullptr, [&](auto WEIGHTED) {
      hipLaunchKernelGGL((moe_combine_kernel<DT(), WEIGHTED()>), dim3(p.grid),
                         dim3(256), 0, s, a.x, a.w, a.slot_of, a.out, a.t, a.k,
                         a.slots, a.h, p.lg);
    });
  });
}

void moe_combine_bwd(const MoePermuteArgs& a, hipStream_t s) {
  const RowPlan p = row_plan(a.slots, a.h / 8);
  by_dtype(a.dtype, [&](auto DT) {
    hipLaunchKernelGGL((moe_combine_bwd_kernel<DT()>), dim3(p.grid), dim3(256),
                       0, s, a.x, a.dout, a.w, a.src_of, a.out, a.dw, a.slots,
                       a.t * a.k, a.k, a.h, p.lg);
  });
}

}  // namespace pa
