// Hand-written bf16 MFMA GEMM for gfx950 (C = op(A) x op(B), fp32
// accumulate, bf16 out) with fused epilogues.
//
// Reference role: paddle/phi/kernels/funcs/blas/blaslt_impl.cu.h +
// matmul_kernel_impl.h:108 (library GEMM), fused_gemm_epilogue_kernel.cu
// (bias+gelu epilogue), fused_linear_param_grad_add_kernel.cu (wgrad
// accumulate) -- all re-derived as native CDNA4 kernels.  A per-shape
// autotune table (paddle_amd/ops/gemm_table.json, the reference's
// matmul_kernel_impl.h:914-958 autotune-between-impls pattern) decides
// own-GEMM vs hipBLASLt per (layout, M, N, K).
//
// Geometry (guide "256^2 8-phase template", counted-vmcnt schedule):
//   * block tile 256x256, K-step 64, 8 waves (2M x 4N), 512 threads
//   * per-wave output 128x64 = acc[8][4] mfma_f32_16x16x32_bf16 frags
//   * LDS: double-buffered A[256][64] + B^T[256][64] bf16 = 128 KiB
//     (1 block/CU -- latency hidden by the phase interleave, not TLP)
//   * 4 phases per K-tile, one C-quadrant (16 MFMA) each, with
//     s_setprio(1) around the MFMA cluster (T5) and two barriers per
//     phase; fragment ds_reads pipelined one phase ahead of their MFMA
//     cluster with counted lgkm waits (A 64 + B 32 + acc 128 regs)
//   * staging for tile t+1 issued during tile t (B at phase 0; A of t+2
//     split into round-pairs at phases 1/3) into the freed LDS slots;
//     the ONLY vmcnt wait is a counted vmcnt(2) at phase 2's end --
//     prefetch loads stay in flight across barriers (T3+T4; never a
//     mid-loop vmcnt(0))
//   * CUTLASS-style tile-group rasterization (GM=8) + XCD chunking so
//     concurrently-resident blocks share A/B panels in L2
//   * st_16x32-style XOR swizzle on LDS rows (T2); XCD-aware bijective
//     workgroup swizzle (T1)
//
// Operand layouts (all producing LDS A[m][k], B'[n][k]):
//   NT: A[M][K] rm, Bt[N][K] rm      (fwd X.W^T; both async-DMA staged)
//   NN: A[M][K] rm, B[K][N] rm       (dgrad dY.W; B reg-transposed)
//   TN: At[K][M] rm, B[K][N] rm      (wgrad dY^T.X; both reg-transposed)
// Epilogues: NONE / BIAS / BIAS_GELU(+aux out) / DGELU(aux in) / ACC.
#include "gemm_common.h"

namespace pa {

#define GEMM_SETPRIO(x) __builtin_amdgcn_s_setprio(x)

// LDS element offset with row-XOR swizzle: rows are 64 bf16 = 128 B; XOR
// the 16B-granule index (elem bits 3..5) with row&7 so a 16-lane column
// slice spreads over 8 bank-slots.
__device__ __forceinline__ unsigned g_swz(unsigned row, unsigned col) {
  return row * 64 + (col ^ ((row & 7u) << 3));
}

enum { LAY_NT = kGemmNT, LAY_NN = kGemmNN, LAY_TN = kGemmTN };
enum { EPI_NONE = kGemmEpiNone, EPI_BIAS = kGemmEpiBias,
       EPI_BIAS_GELU = kGemmEpiBiasGelu, EPI_DGELU = kGemmEpiDGelu };

__device__ __forceinline__ float epi_gelu(float x) {
  // exact-erf GeLU (paddle default approximate=False), same poly as
  // elementwise.hip so fused and unfused paths match bitwise-close
  float z = x * 0.70710678118654752440f;
  float az = fabsf(z);
  float t = 1.f / (1.f + 0.3275911f * az);
  float p = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f +
            t * (-1.453152027f + t * 1.061405429f))));
  float r = 1.f - p * __expf(-az * az);
  float e = copysignf(r, z);
  return 0.5f * x * (1.f + e);
}
__device__ __forceinline__ float epi_gelu_grad(float x) {
  float z = x * 0.70710678118654752440f;
  float az = fabsf(z);
  float t = 1.f / (1.f + 0.3275911f * az);
  float p = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f +
            t * (-1.453152027f + t * 1.061405429f))));
  float r = 1.f - p * __expf(-az * az);
  float e = copysignf(r, z);
  float cdf = 0.5f * (1.f + e);
  float pdf = 0.3989422804014327f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}

// ---------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------
// FAST=true: interior-only instantiation, NT only (grid covers full 256x256
// tiles, K%64==0; no guarded code compiled in -> no spills).  FAST=false:
// guarded boundary kernel launched over the full grid, early-exiting blocks
// the fast launch already covered (skip_interior).
template <int LAYOUT, int EPI, bool ACC, bool FAST>
__launch_bounds__(512, 2)
__global__ void gemm_bf16_kernel(const short* __restrict__ ag, const short* __restrict__ bg,
                                 short* __restrict__ cg, const short* __restrict__ biasg,
                                 short* __restrict__ auxg, int M, int N, int K,
                                 long long lda, long long ldb, long long ldc,
                                 int skip_interior,
                                 long long a_bs = 0, long long b_bs = 0,
                                 long long c_bs = 0) {
  constexpr int BM = 256, BN = 256, BK = 64;
  // batched (grouped-expert) mode: grid.z indexes the batch
  ag += (long long)blockIdx.z * a_bs;
  bg += (long long)blockIdx.z * b_bs;
  cg += (long long)blockIdx.z * c_bs;
  constexpr bool A_DMA = (LAYOUT != LAY_TN);   // A[M][K] row-major
  constexpr bool B_DMA = (LAYOUT == LAY_NT);   // Bt[N][K] row-major
  __shared__ short a_lds[2][BM * BK];
  __shared__ short b_lds[2][BN * BK];

  static_assert(!FAST || LAYOUT == LAY_NT, "the 4-phase pipeline is NT-only");
  static_assert(BM == kGemmTile && BN == kGemmTile, "gemm_common.h tile");

  int row0, col0;
  gemm_tile_origin<FAST>(M, N, row0, col0);
  if (!FAST && skip_interior &&
      row0 + BM <= M && col0 + BN <= N && (K % 64) == 0)
    return;  // covered by the fast launch

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 2;          // 0..1: which 128 rows of C
  const int wc = wid & 3;           // 0..3: which 64 cols of C
  const int l16 = lane & 15;
  const int lg = lane >> 4;

  // DMA staging thread->element map: 4 rounds x (512 thr x 8 elem) per
  // 256x64 tile; round it covers rows [it*64, it*64+64)
  int s_r[4], s_cp[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    int flat = it * 4096 + tid * 8;
    int r = flat / BK, c = flat % BK;
    s_r[it] = r;
    s_cp[it] = c ^ ((r & 7) << 3);   // pre-swizzled source column
  }

  const int nkt = (K + BK - 1) / BK;

  // ---- staging lambdas ----------------------------------------------------
  // A operand, DMA path (A[M][K] row-major; NT/NN).  Rounds r0,r1 only:
  // round r covers tile rows [64r, 64r+64); the fast pipeline stages
  // rounds {0,2} and {1,3} separately (they free after different phases).
  auto stage_a_round = [&](int buf, int kt, int it) {
    const long long k0 = (long long)kt * BK;
    const short* src = ag + (long long)(row0 + s_r[it]) * lda + k0 + s_cp[it];
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)&a_lds[buf][it * 4096 + tid * 8],
        16, 0, 0);
  };
  [[maybe_unused]] auto stage_b_round = [&](int buf, int kt, int it) {
    const long long k0 = (long long)kt * BK;
    const short* src = bg + (long long)(col0 + s_r[it]) * ldb + k0 + s_cp[it];
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)&b_lds[buf][it * 4096 + tid * 8],
        16, 0, 0);
  };
  auto stage_a_dma = [&](int buf, int kt) {
#pragma unroll
    for (int it = 0; it < 4; ++it) stage_a_round(buf, kt, it);
  };
  // B operand, DMA path (Bt[N][K] row-major; NT)
  auto stage_b_dma = [&](int buf, int kt) {
#pragma unroll
    for (int it = 0; it < 4; ++it) stage_b_round(buf, kt, it);
  };
  const int rot = tid & 7;  // staggers transposed LDS writes across banks

  // ---- guarded (boundary / K-tail) staging: zero-fill out of range --------
  // Row-major operand src[limit][K] (A of NT/NN, Bt of NT): tile rows
  // base.. land as LDS rows.
  auto stage_rows = [&](const short* src, long long ld, int limit, int base,
                        short* lds, long long k0) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      int flat = it * 4096 + tid * 8;
      int r = flat / BK, c = flat % BK;
      shortx8 v;
      if (base + r < limit && k0 + c + 7 < K)
        v = *reinterpret_cast<const shortx8*>(src + (long long)(base + r) * ld + k0 + c);
      else
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (base + r < limit && k0 + c + j < K)
                     ? src[(long long)(base + r) * ld + k0 + c + j] : (short)0;
      *reinterpret_cast<shortx8*>(&lds[g_swz(r, c)]) = v;
    }
  };
  // K-major operand src[K][limit] (At of TN, B of NN/TN): read k-rows,
  // scatter-transpose into lds[m|n][k].
  auto stage_transposed = [&](const short* src, long long ld, int limit,
                              int base, short* lds, long long k0) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      int flat = it * 4096 + tid * 8;
      int kr = flat / BN, nc = flat % BN;
      shortx8 v;
      if (k0 + kr < K && base + nc + 7 < limit)
        v = *reinterpret_cast<const shortx8*>(src + (k0 + kr) * ld + base + nc);
      else
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (k0 + kr < K && base + nc + j < limit)
                     ? src[(k0 + kr) * ld + base + nc + j] : (short)0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int i = (j + rot) & 7;
        lds[g_swz(nc + i, kr)] = v[i];
      }
    }
  };
  auto stage_guarded = [&](int buf, int kt) {
    const long long k0 = (long long)kt * BK;
    if (A_DMA) stage_rows(ag, lda, M, row0, a_lds[buf], k0);
    else       stage_transposed(ag, lda, M, row0, a_lds[buf], k0);
    if (B_DMA) stage_rows(bg, ldb, N, col0, b_lds[buf], k0);
    else       stage_transposed(bg, ldb, N, col0, b_lds[buf], k0);
  };

  floatx4 acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = {0.f, 0.f, 0.f, 0.f};

  // fragment registers.  afA/bfA hold the (m0)/(n0) halves, afB/bfB the
  // (m1)/(n1) halves; the fast path software-pipelines reads one phase
  // ahead of their MFMA cluster (counted lgkm waits).
  shortx8 afA[4][2], afB[4][2];  // [mfrag within half][ks]
  shortx8 bfA[2][2], bfB[2][2];  // [nfrag within half][ks]

  auto read_a_half = [&](int buf, int mh, shortx8 (*dst)[2]) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        dst[m][ks] = *reinterpret_cast<const shortx8*>(
            &a_lds[buf][g_swz(wr * 128 + (mh * 4 + m) * 16 + l16, ks * 32 + lg * 8)]);
  };
  auto read_b_half = [&](int buf, int nh, shortx8 (*dst)[2]) {
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        dst[n][ks] = *reinterpret_cast<const shortx8*>(
            &b_lds[buf][g_swz(wc * 64 + (nh * 2 + n) * 16 + l16, ks * 32 + lg * 8)]);
  };
  auto mfma_quadrant = [&](shortx8 (*af)[2], shortx8 (*bf)[2], int mh, int nh) {
    GEMM_SETPRIO(1);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          acc[mh * 4 + m][nh * 2 + n] =
              mfma_bf16(af[m][ks], bf[n][ks], acc[mh * 4 + m][nh * 2 + n]);
    GEMM_SETPRIO(0);
  };

  if constexpr (FAST) {
    // =======================================================================
    // fast path (NT only): 4-phase counted-vmcnt pipeline (T3+T4), T5.
    //
    // Staging runs ahead of consumption so every mid-loop wait is counted:
    //   B(t+1): phase 0 of tile t        (into buf^1; free since t-1 ph3)
    //   A(t+2) rounds {0,2}: phase 1 of t (into buf cur rows freed at ph0)
    //   A(t+2) rounds {1,3}: phase 3 of t (rows freed at ph2)
    //   wait for tile t+1's data: END of tile t phase 3 -- vmcnt(4), the
    //   4 newest (A(t+2)) stay in flight across the barrier.
    // =======================================================================
    // 4-phase counted-vmcnt pipeline, fragment reads one phase ahead.
    // (An 8-phase 2-K-tile variant with fully static banks measured SLOWER
    // -- register-allocator spills in the hot loop; see profiles/ notes.)
    stage_a_dma(0, 0);
    stage_b_dma(0, 0);
    if (nkt > 1) stage_a_dma(1, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // pre-read tile 0's (m0)/(n0) fragments (the pipeline's "prev ph3")
    read_a_half(0, 0, afA);
    read_b_half(0, 0, bfA);

    for (int kt = 0; kt < nkt; ++kt) {
      const int cur = kt & 1;
      const bool pf1 = (kt + 1 < nkt);
      const bool pf2 = (kt + 2 < nkt);

      // ---- phase 0: MFMA (m0,n0); read B(n1); stage B(t+1) ----
      read_b_half(cur, 1, bfB);
      if (pf1) stage_b_dma(cur ^ 1, kt + 1);
      __builtin_amdgcn_s_barrier();
      // afA/bfA (12 reads from prev ph3) must land; bfB's 4 stay in flight
      asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
      mfma_quadrant(afA, bfA, 0, 0);
      __builtin_amdgcn_s_barrier();

      // ---- phase 1: MFMA (m0,n1); read A(m1); stage A(t+2) r0,r2 ----
      read_a_half(cur, 1, afB);
      if (pf2) { stage_a_round(cur, kt + 2, 0); stage_a_round(cur, kt + 2, 2); }
      __builtin_amdgcn_s_barrier();
      asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");  // bfB landed
      mfma_quadrant(afA, bfB, 0, 1);
      __builtin_amdgcn_s_barrier();

      // ---- phase 2: MFMA (m1,n1); counted vmcnt for tile t+1 at end ----
      __builtin_amdgcn_s_barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // afB landed
      mfma_quadrant(afB, bfB, 1, 1);
      if (pf1) {
        // tile t+1's A (staged t-1 ph1/ph3) + B (ph0) must have landed so
        // phase 3 can read them; A(t+2) r0/r2 (2 loads) stay outstanding
        if (pf2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else     asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();

      // ---- phase 3: MFMA (m1,n0); pre-read tile t+1's (m0)/(n0) ----
      if (pf1) read_a_half(cur ^ 1, 0, afA);   // afA free since phase 1
      if (pf2) { stage_a_round(cur, kt + 2, 1); stage_a_round(cur, kt + 2, 3); }
      __builtin_amdgcn_s_barrier();
      mfma_quadrant(afB, bfA, 1, 0);           // inputs already drained
      if (pf1) read_b_half(cur ^ 1, 0, bfA);   // after bfA's last use
      __builtin_amdgcn_s_barrier();
    }
  } else {
    // =======================================================================
    // boundary path: guarded staging, conservative waits
    // =======================================================================
    stage_guarded(0, 0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nkt) stage_guarded(cur ^ 1, kt + 1);
      read_a_half(cur, 0, afA);
      read_b_half(cur, 0, bfA);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      mfma_quadrant(afA, bfA, 0, 0);
      read_b_half(cur, 1, bfB);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      mfma_quadrant(afA, bfB, 0, 1);
      read_a_half(cur, 1, afB);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      mfma_quadrant(afB, bfB, 1, 1);
      mfma_quadrant(afB, bfA, 1, 0);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }

  // ---- epilogue -----------------------------------------------------------
  // bias per output column (bf16), loaded once per nfrag
  float bias_v[4];
  if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) {
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      int col = col0 + wc * 64 + nf * 16 + l16;
      bias_v[nf] = (col < N && biasg) ? bf2f(biasg[col]) : 0.f;
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
        long long idx = (long long)(row + r) * ldc + col;
        float v = acc[m][nf][r];
        if (EPI == EPI_BIAS) {
          v += bias_v[nf];
        } else if (EPI == EPI_BIAS_GELU) {
          v += bias_v[nf];
          if (auxg) auxg[idx] = f2bf(v);
          v = epi_gelu(v);
        } else if (EPI == EPI_DGELU) {
          v *= epi_gelu_grad(bf2f(auxg[idx]));
        }
        if (ACC) v += bf2f(cg[idx]);
        cg[idx] = f2bf(v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host launcher: GemmArgs (api.h) -> one kernel pair of the table
// ---------------------------------------------------------------------------
using GemmBf16Kernel = void (*)(const short*, const short*, short*, const short*,
                                short*, int, int, int, long long, long long,
                                long long, int, long long, long long, long long);
template <int L, int E, bool ACC, bool FAST>
constexpr GemmBf16Kernel kern = gemm_bf16_kernel<L, E, ACC, FAST>;

// The 20 launchable kernels, [layout][variant][fast]; variant is the epilogue,
// or 4 for accumulate.  The 4-phase pipeline is NT-only: NN / TN run the
// guarded kernel over the whole grid (the autotune table keeps them off the
// hot path where hipBLASLt wins).
static const GemmBf16Kernel kGemmBf16Kernels[3][5][2] = {
    {{kern<LAY_NT, EPI_NONE, false, false>, kern<LAY_NT, EPI_NONE, false, true>},
     {kern<LAY_NT, EPI_BIAS, false, false>, kern<LAY_NT, EPI_BIAS, false, true>},
     {kern<LAY_NT, EPI_BIAS_GELU, false, false>, kern<LAY_NT, EPI_BIAS_GELU, false, true>},
     {kern<LAY_NT, EPI_DGELU, false, false>, kern<LAY_NT, EPI_DGELU, false, true>},
     {kern<LAY_NT, EPI_NONE, true, false>, kern<LAY_NT, EPI_NONE, true, true>}},
    {{kern<LAY_NN, EPI_NONE, false, false>, nullptr},
     {kern<LAY_NN, EPI_BIAS, false, false>, nullptr},
     {kern<LAY_NN, EPI_BIAS_GELU, false, false>, nullptr},
     {kern<LAY_NN, EPI_DGELU, false, false>, nullptr},
     {kern<LAY_NN, EPI_NONE, true, false>, nullptr}},
    {{kern<LAY_TN, EPI_NONE, false, false>, nullptr},
     {kern<LAY_TN, EPI_BIAS, false, false>, nullptr},
     {kern<LAY_TN, EPI_BIAS_GELU, false, false>, nullptr},
     {kern<LAY_TN, EPI_DGELU, false, false>, nullptr},
     {kern<LAY_TN, EPI_NONE, true, false>, nullptr}},
};

void gemm_bf16(const GemmArgs& g, hipStream_t s) {
  const auto& pair = kGemmBf16Kernels[g.layout][g.accumulate ? 4 : g.epilogue];
  const GemmPlan plan = gemm_plan(g, 64, pair[1] != nullptr);
  gemm_launch(plan, pair[1], pair[0],
              [&](GemmBf16Kernel k, dim3 grid, int skip_interior) {
    hipLaunchKernelGGL(k, grid, dim3(512), 0, s, (const short*)g.a,
                       (const short*)g.b, (short*)g.c, (const short*)g.bias,
                       (short*)g.aux, (int)g.m, (int)g.n, (int)g.k,
                       (long long)g.lda, (long long)g.ldb, (long long)g.ldc,
                       skip_interior, (long long)g.a_bs, (long long)g.b_bs,
                       (long long)g.c_bs);
  });
}

}  // namespace pa

