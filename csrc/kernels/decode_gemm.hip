// Skinny decode GEMM for gfx950 serving: y[M,N] = x[M,K] @ W[K,N] + bias
// with M <= 32 (a decode micro-batch) -- the shape class where hipBLASLt's
// Tensile tiles reach only ~25% of HBM bandwidth (profiles/
// serve_kernel_stats.csv: 79.6 us for a 134 MB weight read).
//
// Reference role: the decoder GEMM path of fused_multi_transformer
// (paddle/phi/kernels/fusion/gpu/fused_multi_transformer_kernel.cu).
//
// Design: the weight stream IS the kernel -- W[K,N] row-major is read
// exactly once, 16 B/lane coalesced, by the MFMA streamers
// (decode_stream_kernel: bf16 and int8 weights; decode_gemm_int4_kernel).
// Split-K across blocks writes fp32 partials; a tiny second kernel, shared
// by all of them, reduces + adds bias + casts to bf16.
#include "common.h"
#include "api.h"
#include "int4_codes.h"

namespace pa {

// Sum the split-K partials, scale, add bias, cast: y[M,N] bf16.  qinv is the
// weight-code divisor (1 for bf16 weights, 1/127 for int8, 1/7 for int4);
// chscale the per-channel scale of quantized weights, nullptr when there is
// none or the streamer already applied group scales.
__global__ void decode_gemm_reduce_kernel(const float* __restrict__ partial,
                                          const float* __restrict__ chscale,
                                          const short* __restrict__ bias,
                                          short* __restrict__ y, int M, int N,
                                          int mt, int ksplit, float qinv) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)M * N;
  if (i >= total) return;
  int m = (int)(i / N), n = (int)(i % N);
  float acc = 0.f;
  for (int s = 0; s < ksplit; ++s)
    acc += partial[((long long)s * mt + m) * N + n];
  acc *= chscale ? chscale[n] * qinv : qinv;
  if (bias) acc += bf2f(bias[n]);
  y[i] = f2bf(acc);
}

static void launch_reduce(const float* workspace, const float* chscale,
                          float qinv, const void* bias, void* y, int64_t m,
                          int64_t n, int mt, int splits, hipStream_t s) {
  long long total = m * n;
  dim3 rg((unsigned)((total + 255) / 256));
  hipLaunchKernelGGL(decode_gemm_reduce_kernel, rg, dim3(256), 0, s, workspace,
                     chscale, (const short*)bias, (short*)y, (int)m, (int)n,
                     mt, splits, qinv);
}

// ---------------------------------------------------------------------------
// MFMA W-streaming decode GEMM (a vector-ALU inner product is VALU-bound at
// M=32; MFMA makes the arithmetic free so the kernel can run at the
// weight-read roofline).
//
//   y[M,N] = x[M,K] @ W[K,N] + bias,  1 <= M <= 32, N % 256 == 0, K % 64 == 0
//
// One skeleton, decode_stream_kernel<MTILES, Fmt>, for the bf16 and int8
// weight formats; packed int4 is the same pipeline in a kernel of its own
// (decode_gemm_int4_kernel below, which says why).
// W rows are read 16 B/lane coalesced into register sets, converted to bf16
// and TRANSPOSED through LDS (wt[n][k] rows, k-chunk swizzled) so the
// mfma_f32_16x16x32_bf16 B-fragment (8 consecutive k at fixed n -- layout
// verified by probe.hip) is one ds_read_b128.  x is tiny and L2-resident:
// A-fragments load straight from global.  Split-K across grid.y writes fp32
// partials reduced by decode_gemm_reduce_kernel.
//
// Pipeline: DEPTH register sets hold tiles kb+KT .. kb+DEPTH*KT.  At tile kb
// the oldest set is written into LDS buffer cur^1 BEFORE tile kb is
// multiplied from buffer cur, then refilled with tile kb+(DEPTH+1)*KT.  WAR
// on buffer cur (written at the next tile) and RAW on buffer cur^1 (read at
// the next tile) are both cut by the single end-of-tile barrier.  The sets
// are selected at compile time through distinct call sites of one generic
// step in a loop unrolled DEPTH times: a runtime index into a register array
// spills to scratch (measured 960 us vs 50 us).
//
// A weight format supplies what depends on the storage and nothing else:
//   Set, DEPTH        register-set type and prefetch depth -- chosen so that
//                     8 x 16 B loads per thread stay in flight, below which
//                     the kernel is latency-bound, not bandwidth-bound
//   load(set, kb)     global -> registers for the whole tile at kb
//   write(set, wt)    registers -> bf16 in the transposed LDS tile
// ---------------------------------------------------------------------------
constexpr int NB = 256;       // n cols per block
constexpr int KT = 64;        // k rows per LDS tile

// k-chunk swizzle of wt[n][k]: chunk kc (8 bf16) of row n lives at chunk
// kc ^ ((n>>3)&7)
__device__ __forceinline__ int dg_swz(int kc, int n) {
  return (kc ^ ((n >> 3) & 7)) * 8;
}

// byte `j` (0..3) of a dword, sign-extended
__device__ __forceinline__ int q8(unsigned w, int j) { return (int)(w << (24 - 8 * j)) >> 24; }

// The split's accumulators -> partial[ks][MTILES*16][N] fp32.  C lane layout:
// row lg*4+r, col l16; `col` is the lane's column of fragment 0.
template <int MTILES>
__device__ __forceinline__ void store_partial(const floatx4 (&acc)[MTILES][4],
                                              float* __restrict__ partial,
                                              int ks, int N, int col, int lg) {
  const int mt_pad = MTILES * 16;
  float* out = partial + (long long)ks * mt_pad * N;
#pragma unroll
  for (int mt = 0; mt < MTILES; ++mt)
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      int n = col + f * 16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = mt * 16 + lg * 4 + r;
        out[(long long)row * N + n] = acc[mt][f][r];
      }
    }
}

// bf16 rows with row stride ldw.  A 64 x 256 tile is 32 KB = eight 16 B
// loads per thread, so one tile ahead already keeps 8 loads in flight.
// Staging map: 8 rounds x (256 thr x 8 elem); thread covers k row
// r*8 + tid/32 at n segment (tid%32)*8.
struct WBf16 {
  static constexpr int DEPTH = 1;
  typedef shortx8 Set[8];
  const short* w;
  const long long ldw;
  const int s_k, s_n;
  __device__ WBf16(const void* wg, long long ldw_, int, int n0, int tid)
      : ldw(ldw_), s_k(tid >> 5), s_n((tid & 31) * 8) {
    w = (const short*)wg + n0 + s_n;
  }
  __device__ __forceinline__ void load(Set& q, int kb) const {
#pragma unroll
    for (int r = 0; r < 8; ++r)
      q[r] = *reinterpret_cast<const shortx8*>(
          w + (long long)(kb + r * 8 + s_k) * ldw);
  }
  __device__ __forceinline__ void write(const Set& q, short* wt) const {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      int kl = r * 8 + s_k;         // k row within tile
      int kc = kl >> 3, ko = kl & 7;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        wt[(s_n + j) * KT + dg_swz(kc, s_n + j) + ko] = q[r][j];
    }
  }
};

// int8 rows [K, N] contiguous (weight_quantize layout); values convert to
// bf16 at LDS-write time, the per-channel scale/127 applies in the reduce
// kernel.  A tile is 16 KB = four 16 B loads per thread, so TWO tiles ahead
// (depth-1 left the kernel in-flight-limited at ~1.2 TB/s).  Staging map:
// 2 rounds x (k pair, 16 n) per thread -- adjacent k rows pack into ONE b32
// LDS write per n (b16 scatters were the bound: the int8 tile has half the
// bytes but the same element count).
struct WInt8 {
  static constexpr int DEPTH = 2;
  // 16 int8 = 16 n cols of one k row, kept as four dwords: a vector of i8
  // is legalized to one register per element and spilled
  typedef uintx4 Set[4];
  const signed char* w;
  const int n, s_k, s_n;
  __device__ WInt8(const void* wg, long long, int N, int n0, int tid)
      : n(N), s_k((tid >> 4) * 2), s_n((tid & 15) * 16) {
    w = (const signed char*)wg + n0 + s_n;
  }
  __device__ __forceinline__ void load(Set& q, int kb) const {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        q[2 * r + p] = *reinterpret_cast<const uintx4*>(
            w + (long long)(kb + r * 32 + s_k + p) * n);
  }
  __device__ __forceinline__ void write(const Set& q, short* wt) const {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      int kl = r * 32 + s_k;        // even; kl and kl+1 share a chunk
      int kc = kl >> 3, ko = kl & 7;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        int c = s_n + j;
        unsigned lo = (unsigned short)f2bf((float)q8(q[2 * r][j >> 2], j & 3));
        unsigned hi = (unsigned short)f2bf((float)q8(q[2 * r + 1][j >> 2], j & 3));
        *reinterpret_cast<unsigned int*>(
            &wt[c * KT + dg_swz(kc, c) + ko]) = lo | (hi << 16);
      }
    }
  }
};

template <int MTILES, class Fmt>  // MTILES 1: M<=16, 2: M<=32
__launch_bounds__(256, 2)
__global__ void decode_stream_kernel(const short* __restrict__ xg,
                                     const void* __restrict__ wg,
                                     const float*,   // int4 group scales
                                     float* __restrict__ partial,
                                     int M, int N, int K, long long ldw,
                                     int /*gshift*/, int kchunk) {
  __shared__ short wt[2][NB * KT];

  const int n0 = blockIdx.x * NB;
  const int ks = blockIdx.y;
  const int k0 = ks * kchunk;
  const int k1 = min(K, k0 + kchunk);   // k1 - k0 is a multiple of KT

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;      // wave: owns n cols [wv*64, wv*64+64)
  const int l16 = lane & 15;
  const int lg = lane >> 4;

  floatx4 acc[MTILES][4];
#pragma unroll
  for (int mt = 0; mt < MTILES; ++mt)
#pragma unroll
    for (int f = 0; f < 4; ++f)
      acc[mt][f] = floatx4{0.f, 0.f, 0.f, 0.f};

  // x A-fragment rows for this lane (row l16 of each m-tile).  Rows >= M
  // read row M-1 instead: an A row only feeds the same C row, and the
  // reduce kernel never reads C rows >= M.
  int xbase[MTILES];
#pragma unroll
  for (int mt = 0; mt < MTILES; ++mt)
    xbase[mt] = min(mt * 16 + l16, M - 1) * K + lg * 8;

  const Fmt fmt(wg, ldw, N, n0, tid);
  // whole tiles only: kb < k1 implies kb + KT <= k1 <= K
  auto load_w = [&](typename Fmt::Set& q, int kb) {
    if (kb < k1) fmt.load(q, kb);
  };
  auto load_a = [&](shortx8 af[][2], int kb) {
#pragma unroll
    for (int mt = 0; mt < MTILES; ++mt)
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        af[mt][kt] = *reinterpret_cast<const shortx8*>(
            xg + xbase[mt] + kb + kt * 32);
      }
  };

  typename Fmt::Set q[Fmt::DEPTH];
  shortx8 af[MTILES][2], afn[MTILES][2];

  load_w(q[0], k0);
  fmt.write(q[0], wt[0]);
#pragma unroll
  for (int d = 0; d < Fmt::DEPTH; ++d)
    load_w(q[d], k0 + (d + 1) * KT);    // sets 0.. = tiles 1..DEPTH
  load_a(af, k0);
  __syncthreads();

  int cur = 0;
  int kb = k0;
  auto step = [&](typename Fmt::Set& qs) {
    const bool more = kb + KT < k1;
    if (more) {
      fmt.write(qs, wt[cur ^ 1]);
      load_w(qs, kb + (Fmt::DEPTH + 1) * KT);
      load_a(afn, kb + KT);
    }
    // keep the staging phase (conversions, LDS writes, load issue) ahead of
    // the MFMA phase instead of letting the scheduler interleave them
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      int n = wv * 64 + f * 16 + l16;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        int kc = kt * 4 + lg;
        shortx8 bf = *reinterpret_cast<const shortx8*>(
            &wt[cur][n * KT + dg_swz(kc, n)]);
#pragma unroll
        for (int mt = 0; mt < MTILES; ++mt)
          acc[mt][f] = mfma_bf16(af[mt][kt], bf, acc[mt][f]);
      }
    }
    if (more) {
#pragma unroll
      for (int mt = 0; mt < MTILES; ++mt)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) af[mt][kt] = afn[mt][kt];
    }
    cur ^= 1;
    kb += KT;
    __syncthreads();
  };
  while (kb < k1) {
#pragma unroll
    for (int d = 0; d < Fmt::DEPTH; ++d)
      if (kb < k1) step(q[d]);
  }

  store_partial<MTILES>(acc, partial, ks, N, n0 + wv * 64 + l16, lg);
}

// Packed int4 [K/2, N] contiguous (int4_codes.h): the same pipeline at depth
// 4 (a tile is 8 KB = two 16 B loads per thread), kept as a kernel of its own.
// As a format of decode_stream_kernel it measured 3-13% slower HBM-cold
// (int4-gs64 M32 K4096 N12288: 28.8 vs 25.4 us): register allocation of this
// body follows the exact loop form, and the form that suits bf16 / int8
// costs int4 its overlap.  It shares the tile geometry, swizzle, nibble
// helpers, split plan, launcher and reduce kernel with the skeleton.
//
// Nibbles are sign-extended and turned into bf16 in registers (codes -7..7
// are exact in bf16), and one packed byte -- the adjacent-k pair (2kp, 2kp+1)
// at one n -- becomes ONE b32 LDS write.
//
// Scale placement: the LDS tile holds the raw codes.  KT = 64 and
// gs in {64, 128} put every LDS tile inside one group, so the group scale
// is applied to the tile's fp32 MFMA result: acc += tile * scale[g][n].
// That is 4 fp32 FMAs per accumulator fragment and tile (the C layout has
// one n per lane and fragment), cheaper than one multiply per weight at
// LDS-write time, and adds no rounding of the weights.  Scales are indexed
// by the absolute k of the tile, so a split-K boundary may fall inside a
// 128-group.  /7 and per-channel scales stay in the reduce kernel as in int8.

// 16 packed bytes = 16 n cols of one k pair, as four dwords (see WInt8)
typedef uintx4 i4x16;

template <int MTILES, bool GROUPED>  // MTILES 1: M<=16, 2: M<=32
__launch_bounds__(256, 2)
__global__ void decode_gemm_int4_kernel(const short* __restrict__ xg,
                                        const void* __restrict__ wg,
                                        const float* __restrict__ gscale,
                                        float* __restrict__ partial,
                                        int M, int N, int K, long long,
                                        int gshift, int kchunk) {
  const signed char* wq = reinterpret_cast<const signed char*>(wg);
  __shared__ short wt[2][NB * KT];

  const int n0 = blockIdx.x * NB;
  const int ks = blockIdx.y;
  const int k0 = ks * kchunk;
  const int k1 = min(K, k0 + kchunk);   // k1 - k0 is a multiple of KT

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;      // wave: owns n cols [wv*64, wv*64+64)
  const int l16 = lane & 15;
  const int lg = lane >> 4;

  // staging map: 2 rounds x (256 thr x 16 B); thread covers packed row
  // r*16 + tid/16 (k pair 2*that) at n segment (tid%16)*16
  const int s_kp = tid >> 4;
  const int s_n = (tid & 15) * 16;

  floatx4 acc[MTILES][4];
#pragma unroll
  for (int mt = 0; mt < MTILES; ++mt)
#pragma unroll
    for (int f = 0; f < 4; ++f)
      acc[mt][f] = floatx4{0.f, 0.f, 0.f, 0.f};

  // x A-fragment rows for this lane (row l16 of each m-tile).  Rows >= M
  // read row M-1 instead: an A row only feeds the same C row, and the
  // reduce kernel never reads C rows >= M.
  int xbase[MTILES];
#pragma unroll
  for (int mt = 0; mt < MTILES; ++mt)
    xbase[mt] = min(mt * 16 + l16, M - 1) * K + lg * 8;

  // whole tiles only: kb < k1 implies kb + KT <= k1 <= K
  auto load_q = [&](i4x16(&q)[2], int kb) {
    if (kb < k1) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        int kp = (kb >> 1) + r * 16 + s_kp;
        q[r] = *reinterpret_cast<const i4x16*>(wq + (long long)kp * N + n0 + s_n);
      }
    }
  };
  auto write_q = [&](const i4x16(&q)[2], int buf) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      int kl = (r * 16 + s_kp) * 2;   // even; kl and kl+1 share a chunk
      int kc = kl >> 3, ko = kl & 7;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        int n = s_n + j;
        unsigned w = q[r][j >> 2];
        // codes -7..7 are exact in bf16: the cast is the float's top half
        unsigned lo = __float_as_uint((float)q4_lo(w, j & 3)) >> 16;
        unsigned hi = __float_as_uint((float)q4_hi(w, j & 3)) & 0xffff0000u;
        *reinterpret_cast<unsigned int*>(
            &wt[buf][n * KT + dg_swz(kc, n) + ko]) = lo | hi;
      }
    }
  };
  auto load_a = [&](shortx8 af[][2], int kb) {
#pragma unroll
    for (int mt = 0; mt < MTILES; ++mt)
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        af[mt][kt] = *reinterpret_cast<const shortx8*>(
            xg + xbase[mt] + kb + kt * 32);
      }
  };
  // group scale of the tile at absolute k = kb for this lane's 4 C columns
  auto load_s = [&](float (&sc)[4], int kb) {
    if (GROUPED) {
      const float* row = gscale + (long long)(kb >> gshift) * N + n0 + wv * 64 + l16;
#pragma unroll
      for (int f = 0; f < 4; ++f) sc[f] = row[f * 16];
    }
  };

  i4x16 qA[2], qB[2], qC[2], qD[2];
  shortx8 af[MTILES][2], afn[MTILES][2];
  float sc[4] = {1.f, 1.f, 1.f, 1.f};

  load_q(qA, k0);
  write_q(qA, 0);
  load_q(qA, k0 + KT);          // A..D = tiles 1..4 (depth-4 prefetch)
  load_q(qB, k0 + 2 * KT);
  load_q(qC, k0 + 3 * KT);
  load_q(qD, k0 + 4 * KT);
  load_a(af, k0);
  load_s(sc, k0);
  __syncthreads();

  int cur = 0;
  int kb = k0;
  // One barrier per tile, as in decode_stream_kernel: at the tile at kb
  // the set `q` holds tile kb+KT, which goes into buf cur^1 BEFORE tile kb
  // is computed from buf cur; the set is then refilled with tile kb+5*KT.
  auto step = [&](i4x16(&q)[2]) {
    const bool more = kb + KT < k1;
    if (more) {
      write_q(q, cur ^ 1);
      load_q(q, kb + 5 * KT);
      load_a(afn, kb + KT);
    }
    // keep the staging phase (conversions, LDS writes, load issue) ahead of
    // the MFMA phase instead of letting the scheduler interleave them
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      int n = wv * 64 + f * 16 + l16;
      floatx4 t[MTILES];
#pragma unroll
      for (int mt = 0; mt < MTILES; ++mt) t[mt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        int kc = kt * 4 + lg;
        shortx8 bf = *reinterpret_cast<const shortx8*>(
            &wt[cur][n * KT + dg_swz(kc, n)]);
#pragma unroll
        for (int mt = 0; mt < MTILES; ++mt)
          t[mt] = mfma_bf16(af[mt][kt], bf, GROUPED ? t[mt] : acc[mt][f]);
        if (!GROUPED) {
#pragma unroll
          for (int mt = 0; mt < MTILES; ++mt) acc[mt][f] = t[mt];
        }
      }
      if (GROUPED) {
#pragma unroll
        for (int mt = 0; mt < MTILES; ++mt) acc[mt][f] += t[mt] * sc[f];
      }
    }
    if (more) {
#pragma unroll
      for (int mt = 0; mt < MTILES; ++mt)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) af[mt][kt] = afn[mt][kt];
      // next tile's scales: their latency hides behind its staging phase
      load_s(sc, kb + KT);
    }
    cur ^= 1;
    kb += KT;
    __syncthreads();
  };
  while (kb < k1) {
    step(qA);
    if (kb >= k1) break;
    step(qB);
    if (kb >= k1) break;
    step(qC);
    if (kb >= k1) break;
    step(qD);
  }

  store_partial<MTILES>(acc, partial, ks, N, n0 + wv * 64 + l16, lg);
}

// Split plan of the streamer.  ksplit 0 picks the split count: target ~1024
// workgroups, but the fp32 partials cost ksplit*M*N*8 B of write+read, which
// next to int8 / int4 weights rivals the weight stream itself (the reduce
// kernel measured 13% of serving kernel time at the 1024-wg target alone),
// so every split keeps at least kmin k rows (4-8 pipelined LDS tiles; small-N
// shapes take the smaller kmin to reach 2 workgroups per CU).  kchunk is a
// multiple of 64 so every split holds whole LDS tiles.
DecodeSplitPlan decode_split_plan(int64_t k, int64_t n, int64_t ksplit) {
  if (ksplit <= 0) {
    const int64_t nblk = n / NB;
    const int64_t kmin = nblk <= 24 ? 256 : 512;
    ksplit = hmin<int64_t>(1024 / nblk, k / kmin);
  }
  ksplit = hmax<int64_t>(1, hmin<int64_t>(ksplit, k / KT));
  const int64_t kchunk = ((k + ksplit - 1) / ksplit + KT - 1) / KT * KT;
  return {(int)kchunk, (int)((k + kchunk - 1) / kchunk)};
}

// every streamer kernel has this signature; k16 / k32 are the M <= 16 and
// M <= 32 instantiations
typedef void (*StreamKernel)(const short*, const void*, const float*, float*,
                             int, int, int, long long, int, int);

static void launch_stream(StreamKernel k16, StreamKernel k32, const void* x,
                          const void* w, const float* gscale, int gshift,
                          const float* chscale, float qinv, const void* bias,
                          void* y, float* workspace, int64_t m, int64_t n,
                          int64_t k, int64_t ldw, int64_t ksplit,
                          hipStream_t s) {
  const DecodeSplitPlan plan = decode_split_plan(k, n, ksplit);
  const int mt = m <= 16 ? 16 : 32;
  dim3 grid((unsigned)(n / NB), (unsigned)plan.splits);
  hipLaunchKernelGGL(mt == 16 ? k16 : k32, grid, dim3(256), 0, s,
                     (const short*)x, w, gscale, workspace, (int)m, (int)n,
                     (int)k, (long long)ldw, gshift, plan.kchunk);
  launch_reduce(workspace, chscale, qinv, bias, y, m, n, mt, plan.splits, s);
}

void decode_gemm_mfma(const void* x, const void* w, const void* bias, void* y,
                      float* workspace, int64_t m, int64_t n, int64_t k,
                      int64_t ldw, int64_t ksplit, hipStream_t s) {
  launch_stream(decode_stream_kernel<1, WBf16>, decode_stream_kernel<2, WBf16>,
                x, w, nullptr, -1, nullptr, 1.f, bias, y, workspace, m, n, k,
                ldw, ksplit, s);
}

void decode_gemm_int8(const void* x, const void* qw, const float* scale,
                      const void* bias, void* y, float* workspace, int64_t m,
                      int64_t n, int64_t k, int64_t ksplit, hipStream_t s) {
  launch_stream(decode_stream_kernel<1, WInt8>, decode_stream_kernel<2, WInt8>,
                x, qw, nullptr, -1, scale, 1.f / 127.f, bias, y, workspace, m,
                n, k, n, ksplit, s);
}

void decode_gemm_int4(const void* x, const void* qw, const float* scale,
                      const void* bias, void* y, float* workspace, int64_t m,
                      int64_t n, int64_t k, int64_t group_size, int64_t ksplit,
                      hipStream_t s) {
  const int gshift = group_shift(group_size);
  if (gshift >= 0)
    launch_stream(decode_gemm_int4_kernel<1, true>,
                  decode_gemm_int4_kernel<2, true>, x, qw, scale, gshift,
                  nullptr, 1.f / 7.f, bias, y, workspace, m, n, k, n, ksplit, s);
  else
    launch_stream(decode_gemm_int4_kernel<1, false>,
                  decode_gemm_int4_kernel<2, false>, x, qw, nullptr, gshift,
                  scale, 1.f / 7.f, bias, y, workspace, m, n, k, n, ksplit, s);
}

}  // namespace pa
