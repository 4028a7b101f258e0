// MXFP4 weight-only decode GEMM for gfx950 (W4A16):
//   y[M,N] = x[M,K] . dequant(qweight, weight_scale)^T (+ bias),  1 <= M <= 32
// x, y, bias bf16; qweight uint8 e2m1 codes [N, K/2]; weight_scale uint8 e8m0
// [N, K/32] (the format of gemm_mx.hip); fp32 accumulation; x is NOT quantized.
//
// The weight is K-contiguous, so it never touches LDS: one lane's 16-byte load
// is exactly one 32-element MX block of one output row, i.e. after an
// in-register convert four complete mfma_f32_16x16x32_bf16 B operands (8 k
// each) that share one scale byte.
//
// Lane map.  A block is 4 waves x 64 rows = 256 rows of W (N % 64 == 0: the
// last block may leave whole waves idle).  Lane (l16, lg) of a wave owns rows
// n = n_wave + 16 f + l16, f = 0..3.  Per 128-element k-slab it loads bytes
// 16 lg .. 16 lg + 15 of the slab's 64 code bytes = elements 32 lg .. + 31.
// Register c (0..3) of that load converts to the B fragment of MFMA c.  A sum
// over k does not care which eight elements a lane group gives to which MFMA
// as long as A agrees, so MFMA c takes x[m][slab + 32 lg + 8 c .. + 7] from
// lane (l16 = m, lg).
//
// Pipeline.  The unit is a superslab of 4 slabs (512 k): the four loads of one
// (f, superslab) are issued back to back and walk 256 contiguous bytes of each
// of the 16 rows.  Two register sets, Q0 (f = 0, 1) and Q1 (f = 2, 3), of
// 8 x 16 B each, selected at compile time.  While Q0 of superslab t is
// multiplied, Q1(t) is in flight; Q0 is refilled with t + 1 before Q1(t) is
// waited for: at every wait at least 8 weight loads per lane stay in flight.
// The 4-byte scale loads of a set (one dword per (f, slab): the four e8m0 bytes
// of the slab's four blocks, byte lg is the lane's) are issued in front of the
// set's weight loads, so the in-order vmcnt retires them first and they sit
// behind no wait of their own.
//
// x.  Staged once per block and superslab into LDS, [16 MTILES][512] bf16,
// double buffered, the 16-byte chunk index of row r XORed with r & 15; global
// -> registers at the top of a step, registers -> LDS after its MFMAs, one
// barrier per step.  A fragments are ds_read_b128; the 16 lanes of a group
// read 16 different 16-byte slots of the 256-byte bank row (docs/KERNELS.md).
// Rows >= M replicate row M - 1; their C rows are never stored.
//
// Split-K over grid.y writes fp32 partials [splits][16 MTILES][N] (rows < M
// only), summed with the bias by decode_gemm_reduce_kernel.  No atomics.
#include <type_traits>
#include "common.h"
#include "api.h"
#include "decode_gemm.h"

namespace pa {

constexpr int MX_NB = 256;     // W rows per block: 4 waves x 64
constexpr int MX_SLAB = 128;   // k per slab: one 16 B load per lane
constexpr int MX_KS = 512;     // k per superslab: 4 slabs, one register set pair

typedef __attribute__((ext_vector_type(2))) __bf16 mx_bf16x2;

// 8 e2m1 codes (element i in nibble i) x 2^(E - 127), E the exponent field of
// `scale`, as 8 bf16.  v_cvt_scalef32_pk_bf16_fp4 converts one byte: the low
// nibble to the low half.  Exact for scale bytes in [8, 247] (the results are
// normal bf16 numbers or zero); tests/test_decode_gemm_mx_gpu.py reads the
// convert off against the format over all 256 code bytes.
__device__ __forceinline__ shortx8 mx_cvt8(unsigned w, float scale) {
  union { mx_bf16x2 p[4]; shortx8 v; } u;
  u.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
  u.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
  u.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
  u.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
  return u.v;
}

// e8m0 byte -> the fp32 with that exponent field
__device__ __forceinline__ float mx_scale(unsigned byte) {
  return __uint_as_float(byte << 23);
}

template <int MTILES>  // 1: M <= 16, 2: M <= 32
__launch_bounds__(256, 2)
__global__ void decode_gemm_mxfp4_kernel(const short* __restrict__ xg,
                                         const unsigned char* __restrict__ wg,
                                         const unsigned char* __restrict__ sg,
                                         float* __restrict__ partial,
                                         int M, int N, int K, int kchunk) {
  constexpr int ROWS = 16 * MTILES;
  constexpr int XL = ROWS / 4;       // 16 B x chunks per thread and superslab
  __shared__ short xs[2][ROWS * MX_KS];

  const int ks = blockIdx.y;
  const int k0 = ks * kchunk;
  const int k1 = min(K, k0 + kchunk);   // k1 - k0 is a multiple of MX_SLAB

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int l16 = lane & 15;
  const int lg = lane >> 4;
  // N % 64 == 0: a wave of the last block is whole or idle.  An idle wave
  // streams the block's first 64 rows again (in bounds, no branch in the
  // loop) and stores nothing.
  const bool active = blockIdx.x * MX_NB + wv * 64 < N;
  const int n_wave = blockIdx.x * MX_NB + (active ? wv * 64 : 0);

  const long long kbytes = K >> 1;      // code bytes per row
  const int nblk = K >> 5;              // scale bytes per row
  // the lane's row of fragment 0
  const unsigned char* wrow = wg + (long long)(n_wave + l16) * kbytes + lg * 16;
  const unsigned char* srow = sg + (long long)(n_wave + l16) * nblk;

  floatx4 acc[MTILES][4];
#pragma unroll
  for (int mt = 0; mt < MTILES; ++mt)
#pragma unroll
    for (int f = 0; f < 4; ++f)
      acc[mt][f] = floatx4{0.f, 0.f, 0.f, 0.f};

  typedef uintx4 WSet[2][4];       // [f within the pair][slab]
  typedef unsigned SSet[2][4];     // scale dwords, same indices

  // Slabs j < nv = (k1 - kb) / 128 of the superslab at kb are inside [k0, k1).
  // A slab past k1 re-reads slab 0 (kb < k1 <= K: the address is inside the
  // row, the line is in cache) and is never multiplied, so the loads carry no
  // guard and the register sets are always fully defined.
  auto load_set = [&](WSet& q, SSet& sc, auto fb_c, int kb) __attribute__((always_inline)) {
    constexpr int FB = decltype(fb_c)::value;
    const int nv = (k1 - kb) >> 7;
#pragma unroll
    for (int ff = 0; ff < 2; ++ff)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        sc[ff][j] = *reinterpret_cast<const unsigned*>(
            srow + (long long)(FB + ff) * 16 * nblk + (kb >> 5) + (j < nv ? 4 * j : 0));
#pragma unroll
    for (int ff = 0; ff < 2; ++ff)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        q[ff][j] = *reinterpret_cast<const uintx4*>(
            wrow + (long long)(FB + ff) * 16 * kbytes + (kb >> 1) + (j < nv ? 64 * j : 0));
  };

  auto mul_set = [&](const WSet& q, const SSet& sc, auto fb_c, int buf, int nv) __attribute__((always_inline)) {
    constexpr int FB = decltype(fb_c)::value;
    const short* xb = xs[buf];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nv) {
        float s[2];
#pragma unroll
        for (int ff = 0; ff < 2; ++ff)
          s[ff] = mx_scale((sc[ff][j] >> (8 * lg)) & 0xffu);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          shortx8 a[MTILES];
#pragma unroll
          for (int mt = 0; mt < MTILES; ++mt)
            a[mt] = *reinterpret_cast<const shortx8*>(
                &xb[(mt * 16 + l16) * MX_KS + (((16 * j + 4 * lg + c) ^ l16) << 3)]);
#pragma unroll
          for (int ff = 0; ff < 2; ++ff) {
            const shortx8 b = mx_cvt8(q[ff][j][c], s[ff]);
#pragma unroll
            for (int mt = 0; mt < MTILES; ++mt)
              acc[mt][FB + ff] = mfma_bf16(a[mt], b, acc[mt][FB + ff]);
          }
        }
      }
    }
  };
  // x superslab: chunk p = it * 256 + tid is row p / 64, 16-byte chunk p % 64.
  // Rows >= M read row M - 1; a chunk past k1 belongs to a slab that is never
  // multiplied and reads the last chunk of the row instead.
  auto load_x = [&](shortx8 (&xr)[XL], int kb) __attribute__((always_inline)) {
    const int k = min(kb + lane * 8, K - 8);
#pragma unroll
    for (int it = 0; it < XL; ++it)
      xr[it] = *reinterpret_cast<const shortx8*>(
          xg + min(it * 4 + wv, M - 1) * K + k);
  };
  auto write_x = [&](const shortx8 (&xr)[XL], int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < XL; ++it) {
      const int row = it * 4 + wv;
      *reinterpret_cast<shortx8*>(
          &xs[buf][row * MX_KS + ((lane ^ (row & 15)) << 3)]) = xr[it];
    }
  };

  using F0 = std::integral_constant<int, 0>;
  using F2 = std::integral_constant<int, 2>;
  WSet q0, q1;
  SSet s0, s1;
  shortx8 xr[XL];

  load_x(xr, k0);
  load_set(q0, s0, F0{}, k0);
  load_set(q1, s1, F2{}, k0);
  write_x(xr, 0);
  __syncthreads();

  // Steady state: the superslab at kb is whole (kb + 512 < k1), so its
  // multiplies carry no guard; only the last one may hold fewer than 4 slabs.
  // The scheduling barriers keep every phase where it is written: x loads,
  // then Q0's MFMAs, Q0's refill, Q1's MFMAs, Q1's refill, the LDS write.
  int cur = 0, kb = k0;
  for (; kb + MX_KS < k1; kb += MX_KS) {
    load_x(xr, kb + MX_KS);
    __builtin_amdgcn_sched_barrier(0);
    mul_set(q0, s0, F0{}, cur, 4);
    __builtin_amdgcn_sched_barrier(0);
    load_set(q0, s0, F0{}, kb + MX_KS);
    __builtin_amdgcn_sched_barrier(0);
    mul_set(q1, s1, F2{}, cur, 4);
    __builtin_amdgcn_sched_barrier(0);
    load_set(q1, s1, F2{}, kb + MX_KS);
    __builtin_amdgcn_sched_barrier(0);
    write_x(xr, cur ^ 1);
    cur ^= 1;
    // RAW on buffer cur (written above, read in the next step) and WAR on the
    // other one (read above, written in the next step)
    __syncthreads();
  }
  const int nv = (k1 - kb) >> 7;        // 1..4 slabs in the last superslab
  mul_set(q0, s0, F0{}, cur, nv);
  mul_set(q1, s1, F2{}, cur, nv);

  // C lane layout: register r = row 4 lg + r, column l16 of the fragment
  if (active) {
    float* out = partial + (long long)ks * ROWS * N + n_wave + l16;
#pragma unroll
    for (int mt = 0; mt < MTILES; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mt * 16 + lg * 4 + r;
        if (row < M) {
#pragma unroll
          for (int f = 0; f < 4; ++f)
            out[(long long)row * N + f * 16] = acc[mt][f][r];
        }
      }
  }
}

// Split plan: about 1024 workgroups, every split at least kmin k (the smaller
// kmin where there are few row blocks), kchunk a multiple of the 128-k slab.
// The targets are those decode_split_plan documents for the [K, N] streamers;
// docs/KERNELS.md "MXFP4 decode streamer" says what has been measured.
DecodeSplitPlan decode_mx_split_plan(int64_t k, int64_t n, int64_t ksplit) {
  if (ksplit <= 0) {
    const int64_t nblk = (n + MX_NB - 1) / MX_NB;
    const int64_t kmin = nblk <= 24 ? 256 : 512;
    ksplit = hmin<int64_t>(1024 / nblk, k / kmin);
  }
  ksplit = hmax<int64_t>(1, hmin<int64_t>(hmin<int64_t>(ksplit, k / MX_SLAB), 65535));
  const int64_t kchunk =
      ((k + ksplit - 1) / ksplit + MX_SLAB - 1) / MX_SLAB * MX_SLAB;
  return {(int)kchunk, (int)((k + kchunk - 1) / kchunk)};
}

void decode_gemm_mxfp4(const void* x, const void* qw, const void* scales,
                       const void* bias, void* y, float* workspace, int64_t m,
                       int64_t n, int64_t k, int64_t ksplit, hipStream_t s) {
  const DecodeSplitPlan plan = decode_mx_split_plan(k, n, ksplit);
  const int mt = m <= 16 ? 16 : 32;
  dim3 grid((unsigned)((n + MX_NB - 1) / MX_NB), (unsigned)plan.splits);
  hipLaunchKernelGGL(mt == 16 ? decode_gemm_mxfp4_kernel<1>
                              : decode_gemm_mxfp4_kernel<2>,
                     grid, dim3(256), 0, s, (const short*)x,
                     (const unsigned char*)qw, (const unsigned char*)scales,
                     workspace, (int)m, (int)n, (int)k, plan.kchunk);
  decode_gemm_launch_reduce(workspace, nullptr, 1.f, bias, y, m, n, mt,
                            plan.splits, s);
}

// codes [N, K/2] + scales [N, K/32] -> bf16 [N, K] contiguous, for prefill
// shapes (F.linear takes the NT layout as it is).  A lane converts one MX
// block: 16 bytes in, 64 bytes out.
__global__ void mx_dequant_fp4_kernel(const unsigned char* __restrict__ codes,
                                      const unsigned char* __restrict__ scales,
                                      short* __restrict__ out,
                                      long long nblocks) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < nblocks; i += stride) {
    const uintx4 q = *reinterpret_cast<const uintx4*>(codes + i * 16);
    const float sc = mx_scale(scales[i]);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *reinterpret_cast<shortx8*>(out + i * 32 + c * 8) = mx_cvt8(q[c], sc);
  }
}

void mx_dequant_fp4(const void* codes, const void* scales, void* out,
                    int64_t rows, int64_t k, hipStream_t s) {
  const long long nblocks = rows * (k / 32);
  dim3 g((unsigned)elementwise_grid((nblocks + 255) / 256));
  hipLaunchKernelGGL(mx_dequant_fp4_kernel, g, dim3(256), 0, s,
                     (const unsigned char*)codes, (const unsigned char*)scales,
                     (short*)out, nblocks);
}

}  // namespace pa
