// MXFP4 (OCP microscaling: e2m1 elements, one e8m0 scale per 32 elements
// along K) for gfx950: a block-scaled fp4 MFMA GEMM, the bf16 -> MXFP4
// quantizer that feeds it, and the one-wave probe that pins the hardware
// facts both rest on.
//
// Format (public, docs/KERNELS.md "MXFP4 GEMM"):
//   codes  uint8 [R, K/2]: byte i of a row = element 2i in the low nibble,
//          2i+1 in the high one; nibble = sign | 2-bit exponent | 1-bit
//          mantissa, magnitudes {0, .5, 1, 1.5, 2, 3, 4, 6}.
//   scales uint8 [R, K/32] e8m0: 2^(byte - 127).
//
// Hardware facts (mfma_probe_fp4mx, tests/test_gemm_mx_gpu.py::test_probe):
//   v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 4 (e2m1 x e2m1)
//   * operand: lane l holds row l % 16, k-elements 32 * (l / 16) .. +31 as
//     16 bytes in FOUR registers, element 2i in the low nibble of byte i;
//   * C as for 16x16x32: lane l register r = C[4 * (l / 16) + r][l % 16];
//   * scale: lane l supplies the e8m0 byte of exactly its own 32-element
//     block, in the byte of its scale register that the op_sel immediate
//     names (0..3); the other three bytes are not read; 127 = 1.0.
//
// GEMM: C[m][n] = sum_k A[m][k] * B[n][k] (NT), fp32 accumulate, optional
// bf16 bias[n], bf16 C.  256 x 256 block tile, BK = 256 elements = 128 bytes
// per row: the byte geometry of the fp8 [256][128] tile, so the 16-byte
// granule XOR image (row & 7), the 4 x (512 threads x 16 B) DMA rounds and
// the guarded zero-filling staging are those of gemm_fp8.hip.  8 waves as
// 2 x 4, wave tile 128 x 64, two MFMA k-steps per tile; a fragment is one
// ds_read_b128 into 4 registers.
//
// k order inside a tile.  A sum over k does not care which lane group takes
// which 32-element block as long as A and B agree, so lane group lg takes
// blocks 2 * lg and 2 * lg + 1 of the tile's 8 (k-step ks reads byte column
// 32 * lg + 16 * ks) instead of blocks lg and 4 + lg.  The two scale bytes a
// lane needs for one fragment row are then ADJACENT in memory: one 2-byte
// global load per (fragment row, k-tile) puts them in bytes 0 and 1 of one
// register and op_sel = ks picks between them.  Scale path built: straight
// from global, one tile ahead, no LDS image and no VALU extraction (the
// other two options in the design note cost a shift per (fragment, k-step)
// or a second staging pass and its barrier).  The loads are issued BEFORE
// the next tile's operand DMA, so the in-order vmcnt retires them first and
// the only wait they sit behind is the end-of-tile wait the DMA needs anyway.
//
// Main loop: the 2-barrier double-buffered loop of gemm_fp8.hip.  The
// counted-vmcnt 4-phase schedule of gemm.hip has not been tried here.
#include <type_traits>
#include "gemm_common.h"

namespace pa {

typedef __attribute__((ext_vector_type(8))) int intx8;

// e2m1 x e2m1 with per-lane block scales in byte OPSEL of sa / sb
template <int OPSEL>
__device__ __forceinline__ floatx4 mfma_fp4mx(intx4 a, intx4 b, floatx4 c,
                                              int sa, int sb) {
  intx8 a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0};
  intx8 b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a8, b8, c, 4, 4, OPSEL, sa, OPSEL, sb);
}

// ---------------------------------------------------------------------------
// probe: one wave, one MFMA.  a, bt [16][64] codes, sa, sb [16][4] scale
// bytes, c [16][16] fp32.  Lane l puts ITS scale byte (row l % 16, block
// l / 16) into byte OPSEL of the scale register and the row's other three
// bytes into the other positions, so a result that equals the reference
// shows that byte OPSEL of the lane's own register is the one applied.
// ---------------------------------------------------------------------------
template <int OPSEL>
__global__ void mfma_probe_fp4mx_kernel(const unsigned char* __restrict__ a,
                                        const unsigned char* __restrict__ bt,
                                        const unsigned char* __restrict__ sa,
                                        const unsigned char* __restrict__ sb,
                                        float* __restrict__ c) {
  const int lane = threadIdx.x & 63;
  const int l16 = lane & 15, lg = lane >> 4;
  intx4 af = *reinterpret_cast<const intx4*>(a + l16 * 64 + lg * 16);
  intx4 bf = *reinterpret_cast<const intx4*>(bt + l16 * 64 + lg * 16);
  unsigned wa = 0, wb = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int src = (lg + j - OPSEL) & 3;
    wa |= (unsigned)sa[l16 * 4 + src] << (8 * j);
    wb |= (unsigned)sb[l16 * 4 + src] << (8 * j);
  }
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = mfma_fp4mx<OPSEL>(af, bf, acc, (int)wa, (int)wb);
#pragma unroll
  for (int r = 0; r < 4; ++r) c[(lg * 4 + r) * 16 + l16] = acc[r];
}

void mfma_probe_fp4mx(const void* a, const void* bt, const void* sa,
                      const void* sb, float* c, int opsel, hipStream_t s) {
  using Kernel = decltype(&mfma_probe_fp4mx_kernel<0>);
  const Kernel k[4] = {mfma_probe_fp4mx_kernel<0>, mfma_probe_fp4mx_kernel<1>,
                       mfma_probe_fp4mx_kernel<2>, mfma_probe_fp4mx_kernel<3>};
  hipLaunchKernelGGL(k[opsel & 3], dim3(1), dim3(64), 0, s,
                     (const unsigned char*)a, (const unsigned char*)bt,
                     (const unsigned char*)sa, (const unsigned char*)sb, c);
}

// ---------------------------------------------------------------------------
// quantizer: bf16 [R, K] (row stride ld) -> codes + scales in one read pass.
// A lane owns 8 consecutive elements (one 16-byte load), four lanes own a
// block; amax is the integer max of the magnitude bits, combined across the
// four lanes by two cross-lane steps.  The rule (finite inputs):
//   E = biased fp32 exponent of amax; scale byte = max(E, 2) - 2, i.e.
//   e = floor(log2 amax) - 2 clamped below at -127 (E <= 254 keeps it under
//   125); amax == 0 -> byte 127, zero codes; element = x * 2^-e rounded to
//   the nearest e2m1 value, ties to the even code, saturating at 6.
// The rounding is integer code on the fp32 bits, not v_cvt_scalef32_pk_fp4:
// the convert's rounding and saturation have not been read off against the
// rule on hardware, and the rule is what the format promises.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned e2m1_code(short xb, float inv_scale) {
  const float y = bf2f((short)(xb & 0x7fff)) * inv_scale;   // |x| * 2^-e < 8
  unsigned bits = __float_as_uint(y);
  // y >= 1: round the 23-bit mantissa to 1 bit, nearest even; the carry runs
  // into the exponent.  (exponent, mantissa bit) - (127, 0) + 2 is the code.
  unsigned hi = ((bits + 0x1fffffu + ((bits >> 22) & 1u)) >> 22) - 252u;
  // y < 1: grid {0, .5, 1}; adding 2^22 leaves round-to-nearest-even(2y) in
  // the low mantissa bits
  unsigned lo = __float_as_uint(y + 4194304.0f) & 3u;
  unsigned code = y < 1.0f ? lo : (hi < 7u ? hi : 7u);
  return code | (((unsigned)(unsigned short)xb >> 12) & 8u);
}

__global__ void mx_quant_fp4_kernel(const short* __restrict__ x,
                                    unsigned char* __restrict__ codes,
                                    unsigned char* __restrict__ scales,
                                    long long rows, int k8, long long ld) {
  // k8 = K / 8 lanes per row, a multiple of 4: a quad of lanes never
  // straddles a row or the end of the tensor, and the grid stride keeps quads
  const long long n8 = rows * k8;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n8; i += stride) {
    const long long r = i / k8;
    const int c8 = (int)(i - r * k8);
    const shortx8 v = *reinterpret_cast<const shortx8*>(x + r * ld + (long long)c8 * 8);
    int amax = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = max(amax, (int)(v[j] & 0x7fff));
    amax = max(amax, __shfl_xor(amax, 1, WAVE));
    amax = max(amax, __shfl_xor(amax, 2, WAVE));
    const int ex = amax >> 7;                        // biased exponent
    const int sbyte = amax == 0 ? 127 : max(ex, 2) - 2;
    // 2^-e = 2^(127 - sbyte): biased exponent 254 - sbyte, in [2, 254]
    const float inv_scale = __uint_as_float((unsigned)(254 - sbyte) << 23);
    unsigned packed = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) packed |= e2m1_code(v[j], inv_scale) << (4 * j);
    *reinterpret_cast<unsigned*>(codes + r * (4LL * k8) + 4LL * c8) = packed;
    if ((c8 & 3) == 0) scales[r * (k8 >> 2) + (c8 >> 2)] = (unsigned char)sbyte;
  }
}

void mx_quant_fp4(const void* x, void* codes, void* scales, int64_t rows,
                  int64_t k, int64_t ld, hipStream_t s) {
  const long long n8 = rows * (k / 8);
  dim3 g((unsigned)hmin<long long>((n8 + 255) / 256, 4096));
  hipLaunchKernelGGL(mx_quant_fp4_kernel, g, dim3(256), 0, s, (const short*)x,
                     (unsigned char*)codes, (unsigned char*)scales,
                     (long long)rows, (int)(k / 8), (long long)ld);
}

// ---------------------------------------------------------------------------
// GEMM.  All k quantities inside the kernel are BYTES of codes (Kb = K / 2,
// tile 128 B); scale rows are indexed in blocks (K / 32 per row, 8 per tile).
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned mx_swz(unsigned row, unsigned bcol) {
  return row * 128 + (bcol ^ ((row & 7u) << 4));
}

template <bool FAST>
__launch_bounds__(512, 2)
__global__ void gemm_mxfp4_kernel(const unsigned char* __restrict__ ag,
                                  const unsigned char* __restrict__ bg,
                                  const unsigned char* __restrict__ sag,
                                  const unsigned char* __restrict__ sbg,
                                  short* __restrict__ cg,
                                  const short* __restrict__ biasg,
                                  int M, int N, int Kb,
                                  long long lda, long long ldb, long long ldc,
                                  long long ldsa, long long ldsb,
                                  int skip_interior, int has_bias) {
  constexpr int BM = 256, BN = 256, BK = 128;   // BK in bytes = 256 elements
  __shared__ unsigned char a_lds[2][BM * BK];
  __shared__ unsigned char b_lds[2][BN * BK];

  static_assert(BM == kGemmTile && BN == kGemmTile, "gemm_common.h tile");
  int row0, col0;
  gemm_tile_origin<FAST>(M, N, row0, col0);
  if (!FAST && skip_interior &&
      row0 + BM <= M && col0 + BN <= N && (Kb % BK) == 0)
    return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 2;
  const int wc = wid & 3;
  const int l16 = lane & 15;
  const int lg = lane >> 4;

  // DMA staging map: 4 rounds x (512 thr x 16 B); round r covers 64 rows
  int s_r[4], s_cp[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    int fb = it * 8192 + tid * 16;
    int r = fb / BK, c = fb % BK;
    s_r[it] = r;
    s_cp[it] = c ^ ((r & 7) << 4);
  }
  const int nkt = (Kb + BK - 1) / BK;
  const int nblk = Kb / 16;                      // scale bytes per row

  auto stage_dma = [&](int buf, int kt) {
    const long long k0 = (long long)kt * BK;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const unsigned char* src = ag + (long long)(row0 + s_r[it]) * lda + k0 + s_cp[it];
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)&a_lds[buf][it * 8192 + tid * 16],
          16, 0, 0);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const unsigned char* src = bg + (long long)(col0 + s_r[it]) * ldb + k0 + s_cp[it];
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)&b_lds[buf][it * 8192 + tid * 16],
          16, 0, 0);
    }
  };
  // Kb is a multiple of 64, so a 16-byte chunk is wholly inside or outside
  auto stage_guarded = [&](int buf, int kt) {
    const long long k0 = (long long)kt * BK;
    for (int fb = tid * 16; fb < BM * BK; fb += 512 * 16) {
      const int r = fb / BK, c = fb % BK;
      const bool k_in = k0 + c < Kb;
      intx4 va = {0, 0, 0, 0}, vb = {0, 0, 0, 0};
      if (k_in && row0 + r < M)
        va = *reinterpret_cast<const intx4*>(ag + (long long)(row0 + r) * lda + k0 + c);
      if (k_in && col0 + r < N)
        vb = *reinterpret_cast<const intx4*>(bg + (long long)(col0 + r) * ldb + k0 + c);
      *reinterpret_cast<intx4*>(&a_lds[buf][mx_swz(r, c)]) = va;
      *reinterpret_cast<intx4*>(&b_lds[buf][mx_swz(r, c)]) = vb;
    }
  };

  // scales of one k-tile: per fragment row the two bytes of blocks
  // 8 * kt + 2 * lg, + 1 (K / 32 is a multiple of 4: both or neither exist)
  int sa_cur[8], sb_cur[4], sa_nxt[8], sb_nxt[4];
  auto load_scales = [&](int kt, int* sa_r, int* sb_r) {
    const int blk = 8 * kt + 2 * lg;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int row = row0 + wr * 128 + m * 16 + l16;
      const bool ok = FAST || (row < M && blk < nblk);
      sa_r[m] = ok ? (int)*reinterpret_cast<const unsigned short*>(
                         sag + (long long)row * ldsa + blk) : 0x7f7f;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int row = col0 + wc * 64 + n * 16 + l16;
      const bool ok = FAST || (row < N && blk < nblk);
      sb_r[n] = ok ? (int)*reinterpret_cast<const unsigned short*>(
                         sbg + (long long)row * ldsb + blk) : 0x7f7f;
    }
  };

  floatx4 acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = {0.f, 0.f, 0.f, 0.f};

  intx4 afA[4], afB[4];   // A(m0) / A(m1), 4 mfrags each
  intx4 bfA[2], bfB[2];   // B(n0) / B(n1), 2 nfrags each

  auto read_a_half = [&](int buf, int ks, int mh, intx4* dst) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      unsigned row = wr * 128 + (mh * 4 + m) * 16 + l16;
      dst[m] = *reinterpret_cast<const intx4*>(&a_lds[buf][mx_swz(row, lg * 32 + ks * 16)]);
    }
  };
  auto read_b_half = [&](int buf, int ks, int nh, intx4* dst) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      unsigned row = wc * 64 + (nh * 2 + n) * 16 + l16;
      dst[n] = *reinterpret_cast<const intx4*>(&b_lds[buf][mx_swz(row, lg * 32 + ks * 16)]);
    }
  };
  auto mfma_quadrant = [&](auto ks_c, intx4* af, intx4* bf, int mh, int nh) {
    constexpr int KS = decltype(ks_c)::value;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
        acc[mh * 4 + m][nh * 2 + n] = mfma_fp4mx<KS>(
            af[m], bf[n], acc[mh * 4 + m][nh * 2 + n],
            sa_cur[mh * 4 + m], sb_cur[nh * 2 + n]);
    __builtin_amdgcn_s_setprio(0);
  };
  auto k_step = [&](auto ks_c, int cur) {
    constexpr int KS = decltype(ks_c)::value;
    read_a_half(cur, KS, 0, afA);
    read_b_half(cur, KS, 0, bfA);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    mfma_quadrant(ks_c, afA, bfA, 0, 0);
    read_b_half(cur, KS, 1, bfB);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    mfma_quadrant(ks_c, afA, bfB, 0, 1);
    read_a_half(cur, KS, 1, afB);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    mfma_quadrant(ks_c, afB, bfB, 1, 1);
    mfma_quadrant(ks_c, afB, bfA, 1, 0);
  };

  auto stage = [&](int buf, int kt) {
    if constexpr (FAST) stage_dma(buf, kt);
    else stage_guarded(buf, kt);
  };
  auto wait_staged = [&]() {
    if constexpr (FAST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
  };
  using K0 = std::integral_constant<int, 0>;
  using K1 = std::integral_constant<int, 1>;

  load_scales(0, sa_nxt, sb_nxt);
  stage(0, 0);
  wait_staged();
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
#pragma unroll
    for (int m = 0; m < 8; ++m) sa_cur[m] = sa_nxt[m];
#pragma unroll
    for (int n = 0; n < 4; ++n) sb_cur[n] = sb_nxt[n];
    if (kt + 1 < nkt) {
      load_scales(kt + 1, sa_nxt, sb_nxt);   // ahead of the DMA in vmcnt order
      stage(cur ^ 1, kt + 1);
    }
    k_step(K0{}, cur);
    k_step(K1{}, cur);
    wait_staged();
  }

  // epilogue: optional bias, guarded bf16 store
  float bias_v[4];
  if (has_bias) {
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      int col = col0 + wc * 64 + nf * 16 + l16;
      bias_v[nf] = (col < N) ? bf2f(biasg[col]) : 0.f;
    }
  }
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    int row = row0 + wr * 128 + m * 16 + (lg * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (row + r >= M) continue;
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        int col = col0 + wc * 64 + nf * 16 + l16;
        if (col >= N) continue;
        float v = acc[m][nf][r];
        if (has_bias) v += bias_v[nf];
        cg[(long long)(row + r) * ldc + col] = f2bf(v);
      }
    }
  }
}

void gemm_mxfp4(const GemmArgs& g, const uint8_t* sa, const uint8_t* sb,
                int64_t ldsa, int64_t ldsb, hipStream_t s) {
  using Kernel = decltype(&gemm_mxfp4_kernel<true>);
  gemm_launch(gemm_plan(g, 256, true), Kernel(gemm_mxfp4_kernel<true>),
              Kernel(gemm_mxfp4_kernel<false>),
              [&](Kernel k, dim3 grid, int skip_interior) {
    hipLaunchKernelGGL(k, grid, dim3(512), 0, s, (const unsigned char*)g.a,
                       (const unsigned char*)g.b, sa, sb, (short*)g.c,
                       (const short*)g.bias, (int)g.m, (int)g.n,
                       (int)(g.k / 2), (long long)g.lda, (long long)g.ldb,
                       (long long)g.ldc, (long long)ldsa, (long long)ldsb,
                       skip_interior, g.bias != nullptr);
  });
}

}  // namespace pa
