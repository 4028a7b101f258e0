// Weight-only int4 decode: group-scaled int4 MFMA W-streamer + dequantizer.
//
//   y[M,N] (bf16) = x[M,K] (bf16) @ dequant(qw) + bias
//   M <= 32, N % 256 == 0, K % 64 == 0, group_size in {-1, 64, 128}
//
// Storage (paddle_amd.quantization.weight_quantize, "weight_only_int4"):
//   qw    int8 [K/2, N] row-major; byte (kp, n) = (q[2kp, n] & 0xF) |
//         ((q[2kp+1, n] & 0xF) << 4), two's-complement nibbles, codes -7..7
//   scale fp32 [N] (per channel) or [K/gs, N] (groups of gs k rows)
//   w[k, n] ~ q[k, n] * scale[k / gs, n] / 7
//
// Same family as decode_gemm_mfma_kernel (decode_gemm.hip): the packed W
// rows are read 16 B/lane coalesced, nibbles are sign-extended and turned
// into bf16 in registers (codes -7..7 are exact in bf16), and one packed
// byte -- the adjacent-k pair (2kp, 2kp+1) at one n -- becomes ONE b32
// write into the k-chunk-swizzled transposed LDS tile wt[n][k].  The MFMA
// B-fragment is then one ds_read_b128, split-K partials are fp32, and a
// small reduce kernel adds them up, applies /7 (and the per-channel scale),
// adds bias and casts.
//
// Scale placement: the LDS tile holds the raw codes.  KT = 64 and
// gs in {64, 128} put every LDS tile inside one group, so the group scale
// is applied to the tile's fp32 MFMA result: acc += tile * scale[g][n].
// That is 4 fp32 FMAs per accumulator fragment and tile (the C layout has
// one n per lane and fragment), cheaper than one multiply per weight at
// LDS-write time, and adds no rounding of the weights.  Scales are indexed
// by the absolute k of the tile, so a split-K boundary may fall inside a
// 128-group.  Per-channel scales stay in the reduce kernel as in int8.
//
// Bytes in flight: a 64 x 256 int4 tile is 8 KB = two 16 B loads per
// thread, half of the int8 tile.  The int8 kernel needed 8 loads per
// thread outstanding (2 tiles of 4) to leave the latency-bound regime, so
// this kernel prefetches FOUR tiles ahead (4 sets x 2 loads).  The sets
// are named arrays picked at compile time through distinct call sites of
// one generic step in a loop unrolled by four (a runtime-indexed register
// array spills to scratch).
#include "common.h"
#include "api.h"

namespace pa {

namespace {

// 16 packed bytes = 16 n cols of one k pair, kept as four dwords: a vector of
// i8 is legalized to one register per element and spilled
typedef uintx4 i4x16;

// k-chunk swizzle of the transposed tile, as in decode_gemm.hip: chunk kc
// (8 bf16) of row n lives at chunk kc ^ ((n>>3)&7).
__device__ __forceinline__ int q4_swz(int kc, int n) {
  return (kc ^ ((n >> 3) & 7)) * 8;
}

// low / high nibble of byte `j` (0..3) of a dword, sign-extended
__device__ __forceinline__ int q4_lo(unsigned w, int j) { return (int)(w << (28 - 8 * j)) >> 28; }
__device__ __forceinline__ int q4_hi(unsigned w, int j) { return (int)(w << (24 - 8 * j)) >> 28; }

template <int MTILES, bool GROUPED>  // MTILES 1: M<=16, 2: M<=32
__launch_bounds__(256, 2)
__global__ void decode_gemm_int4_kernel(const short* __restrict__ xg,
                                        const signed char* __restrict__ wq,
                                        const float* __restrict__ gscale,
                                        float* __restrict__ partial,
                                        int M, int N, int K, int gshift,
                                        int kchunk) {
  constexpr int NB = 256;       // n cols per block
  constexpr int KT = 64;        // k rows per LDS tile (32 packed rows)
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
            &wt[buf][n * KT + q4_swz(kc, n) + ko]) = lo | hi;
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
  // One barrier per tile, as in decode_gemm_mfma_kernel: at the tile at kb
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
            &wt[cur][n * KT + q4_swz(kc, n)]);
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

  // partial[ks][mt_pad][N] fp32; C lane layout: row lg*4+r, col l16
  const int mt_pad = MTILES * 16;
  float* out = partial + (long long)ks * mt_pad * N;
#pragma unroll
  for (int mt = 0; mt < MTILES; ++mt)
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      int n = n0 + wv * 64 + f * 16 + l16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = mt * 16 + lg * 4 + r;
        out[(long long)row * N + n] = acc[mt][f][r];
      }
    }
}

// sum the split-K partials, apply /7 (and the per-channel scale when the
// streamer did not apply group scales), add bias, cast: y[M,N] bf16
__global__ void decode_gemm_int4_reduce_kernel(const float* __restrict__ partial,
                                               const float* __restrict__ chscale,
                                               const short* __restrict__ bias,
                                               short* __restrict__ y, int M,
                                               int N, int mt, int ksplit) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)M * N;
  if (i >= total) return;
  int m = (int)(i / N), n = (int)(i % N);
  float acc = 0.f;
  for (int s = 0; s < ksplit; ++s)
    acc += partial[((long long)s * mt + m) * N + n];
  acc *= chscale ? chscale[n] * (1.f / 7.f) : (1.f / 7.f);
  if (bias) acc += bf2f(bias[n]);
  y[i] = f2bf(acc);
}

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

inline int group_shift(int64_t group_size) {
  return group_size == 64 ? 6 : (group_size == 128 ? 7 : -1);
}

}  // namespace

int64_t decode_gemm_int4_splits(int64_t k, int64_t ksplit) {
  ksplit = hmax<int64_t>(1, hmin<int64_t>(ksplit, k / 64));
  const int64_t kchunk = ((k + ksplit - 1) / ksplit + 63) / 64 * 64;
  return (k + kchunk - 1) / kchunk;
}

void decode_gemm_int4(const void* x, const void* qw, const float* scale,
                      const void* bias, void* y, float* workspace, int64_t m,
                      int64_t n, int64_t k, int64_t group_size, int64_t ksplit,
                      hipStream_t s) {
  const int mt = m <= 16 ? 16 : 32;
  ksplit = hmax<int64_t>(1, hmin<int64_t>(ksplit, k / 64));
  // kchunk: multiple of 64 so every split holds whole LDS tiles
  const int kchunk = (int)(((k + ksplit - 1) / ksplit + 63) / 64 * 64);
  const int ks = (int)((k + kchunk - 1) / kchunk);
  const int gshift = group_shift(group_size);
  dim3 grid((unsigned)(n / 256), (unsigned)ks);
#define DGQ(MT, GR)                                                           \
  hipLaunchKernelGGL((decode_gemm_int4_kernel<MT, GR>), grid, dim3(256), 0,   \
                     s, (const short*)x, (const signed char*)qw, scale,       \
                     workspace, (int)m, (int)n, (int)k, gshift, kchunk)
  if (gshift >= 0) { if (mt == 16) DGQ(1, true); else DGQ(2, true); }
  else             { if (mt == 16) DGQ(1, false); else DGQ(2, false); }
#undef DGQ
  long long total = m * n;
  dim3 rg((unsigned)((total + 255) / 256));
  hipLaunchKernelGGL(decode_gemm_int4_reduce_kernel, rg, dim3(256), 0, s,
                     workspace, gshift >= 0 ? nullptr : scale,
                     (const short*)bias, (short*)y, (int)m, (int)n, mt, ks);
}

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
