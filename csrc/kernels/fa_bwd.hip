// FlashAttention-2 backward for gfx950 (CDNA4): bf16, head_dim 64 / 128,
// causal or full, dense or varlen, h a multiple of hkv (GQA: q head h reads
// K/V head h / (h/hkv), as in the forward).  The forward is in fa_fwd32.hip,
// the shared pieces in fa_common.h.
//
// No atomics; S is recomputed from Q, K and the saved LSE per FA2.  Kernels:
//   * fa_bwd_delta_kernel: delta[row] = sum_d dO * O.
//   * fa_bwd_dkv_kernel: dK and dV of the dense path without mask and
//     dropout.  MFMA 16x16x32, 8 waves, a 128-row KV block per block; Q / dO
//     staged once per tile by DMA into one image that is read by rows
//     (ds_read_b128) and by columns (ds_read_b64_tr_b16), two buffers so the
//     next tile loads under this tile's math (see the kernel).
//   * fa_bwd_dkv32_kernel: dK or dV (one launch each) for mask, dropout and
//     varlen.  MFMA 32x32x16, 4 waves.
//   * fa_bwd_dq32_kernel: dQ for every path.  MFMA 32x32x16, 4 waves, the
//     forward's swapped layout and its double-buffered K / V image, K read
//     by rows and by columns.
// GQA (hkv != h, no mask) is a compile-time flavour of the three MFMA kernels;
// the GQA = false instantiations are the hkv == h kernels unchanged.  A dK/dV
// block owns a kv block of ONE kv head and G consecutive q heads of its group
// and streams their q tiles, head after head, past the same K/V fragments and
// the same fp32 accumulators: one K/V read, one fp32 sum, one rounding.
// G == h/hkv writes bf16 dK/dV; G < h/hkv (more blocks for small grids) writes
// fp32 partials [b, h/G, skv, d] that fa_bwd_gqa_reduce_kernel sums in fixed
// order.  No atomics.  hkv != h with a mask is refused by the binding.
#include "fa_common.h"

namespace pa {

// ---------------------------------------------------------------------------
// backward: delta[row] = sum_d dO*O
// ---------------------------------------------------------------------------
template <int D>
__global__ void fa_bwd_delta_kernel(const short* __restrict__ dog, const short* __restrict__ og,
                                    float* __restrict__ delta, int H, int Sq,
                                    long long rows,
                                    long long do_sb, long long do_sh, long long do_ss,
                                    long long o_sb, long long o_sh, long long o_ss) {
  // D/8 lanes per row (one 16 B load each), 256/(D/8) rows per block pass,
  // 4 passes in flight.  Rows are walked in memory order: h fastest for the
  // [B, S, H, D] strides of the packed-QKV / varlen paths (h_fast), s
  // fastest for contiguous [B, H, S, D]; delta keeps its [B, H, Sq] order.
  constexpr int LPR = D / 8, RPP = 256 / LPR, UNR = 4;
  const int sub = threadIdx.x % LPR;
  const int rin = threadIdx.x / LPR;
  const bool h_fast = do_sh < do_ss;
  for (long long r0 = (long long)blockIdx.x * (RPP * UNR); r0 < rows;
       r0 += (long long)gridDim.x * (RPP * UNR)) {
    shortx8 a[UNR], bb[UNR];
    long long di[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long long r = r0 + u * RPP + rin;
      di[u] = -1;
      if (r < rows) {
        int sq, h, b;
        if (h_fast) {
          h = (int)(r % H);
          sq = (int)((r / H) % Sq);
        } else {
          sq = (int)(r % Sq);
          h = (int)((r / Sq) % H);
        }
        b = (int)(r / ((long long)Sq * H));
        di[u] = ((long long)b * H + h) * Sq + sq;
        a[u] = *reinterpret_cast<const shortx8*>(
            dog + b * do_sb + h * do_sh + sq * do_ss + sub * 8);
        bb[u] = *reinterpret_cast<const shortx8*>(
            og + b * o_sb + h * o_sh + sq * o_ss + sub * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float acc = 0.f;
      if (di[u] >= 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += bf2f(a[u][k]) * bf2f(bb[u][k]);
      }
#pragma unroll
      for (int off = LPR / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
      if (sub == 0 && di[u] >= 0) delta[di[u]] = acc;
    }
  }
}

// also bound on its own for tests and benchmarks
void flash_attn_bwd_delta(const void* dout, const void* o, float* delta,
                          int64_t b, int64_t h, int64_t sq, int64_t dh,
                          const FaStride& dos, const FaStride& os, hipStream_t s) {
  const long long rows = (long long)b * h * sq;
  const int rows_per_iter = (256 / (int)(dh / 8)) * 4;
  dim3 dgrid((unsigned)hmin<long long>(2048LL, (rows + rows_per_iter - 1) / rows_per_iter));
  if (dh == 128)
    hipLaunchKernelGGL((fa_bwd_delta_kernel<128>), dgrid, dim3(256), 0, s,
                       (const short*)dout, (const short*)o, delta, (int)h,
                       (int)sq, rows, dos.b, dos.h, dos.s, os.b, os.h, os.s);
  else
    hipLaunchKernelGGL((fa_bwd_delta_kernel<64>), dgrid, dim3(256), 0, s,
                       (const short*)dout, (const short*)o, delta, (int)h,
                       (int)sq, rows, dos.b, dos.h, dos.s, os.b, os.h, os.s);
}

// ---------------------------------------------------------------------------
// backward dK/dV: block owns a 128-row KV block; waves own 16 kv rows each;
// iterate 64-row q tiles.  S^T computed as K·Q^T so kv is the C-row.
//
// Q and dO are staged once per tile, by DMA, in ONE LDS image that serves
// both kinds of read: ds_read_b128 rows for the B operand of S^T / dP^T
// (k = d) and ds_read_b64_tr_b16 for the B operand of dV / dK (k = q), so no
// transposed copy is built.  The image is the natural [64][D] tile with the
// 16-byte chunk index of each row XORed by dkv_swz(row); the DMA lands it
// through the same XOR on its source column.  Two {Q, dO} buffers: tile t+1
// is in flight while tile t is computed, one barrier per tile.  P^T and dS^T
// cross a per-wave [q][kv] image as packed 8-byte rows and come back as A
// fragments by transposed reads.  Every MFMA gets the operands, in the k
// order, of the kernel this replaces, so dK / dV are bit-identical to it.
// ---------------------------------------------------------------------------

// chunk-index XOR of row `row` of the [64][D] image.  Bank rule: a 256-byte
// bank row; ds_read_b64_tr_b16 conflicts inside a 32-lane half, ds_read_b128
// inside its 16-lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32).
//   transposed read: a half takes rows 8g+4h+{0..3} of two 16-lane groups
//     g, g+1, 32 bytes per row, the same chunk pair 2*dt, 2*dt+1 -> the 8
//     rows must land on 8 different 32-byte pairs;
//   row read (16x16x32 B operand): a group takes rows {0-3,12-15} at chunk c
//     and rows {4-11} at chunk c^1 (or the other way round) -> 16 slots.
// D = 128: pair bits from row&3 and (row>>3)&1, bit 0 clear.  Rows r and r+4
// share a pair and differ in c's bit 0, so both reads are conflict-free (the
// guide's T10 image (b), bits 1:0 = (row>>2)&3, is 2-way on this row read),
// and rows +4 / +32 keep the XOR, so the second half of a B fragment and the
// next k-step are immediate offsets from one address register per d tile.
// D = 64 has two rows per bank row: row&1 picks the half, (row>>1)&1 and
// (row>>3)&1 the pair inside it; the same two properties hold.
template <int D>
__device__ __forceinline__ unsigned dkv_swz(unsigned row) {
  if constexpr (D == 128)
    return ((row & 3u) << 2) | (((row >> 3) & 1u) << 1);
  else
    return (((row >> 1) & 1u) << 2) | (((row >> 3) & 1u) << 1);
}

// byte offset of 16-byte chunk `ch` of row `row`; stores and both kinds of
// read go through it
template <int D>
__device__ __forceinline__ unsigned dkv_off(unsigned row, unsigned ch) {
  return row * (D * 2) + ((ch ^ dkv_swz<D>(row)) << 4);
}

// ds_read_b64_tr_b16: per 16-lane group, lane 4q+p passes the address of row
// q, columns 4p..4p+3 of a 4-row x 16-column block; lane i gets column i,
// row j in element j.  EXEC must be all ones at every one of these.
//
// The transposed reads are inline asm that ends in its own lgkmcnt(0): as a
// builtin each read was waited for on its own in front of its MFMA, and the
// first one of a tile drew a vmcnt(0) that drained the prefetch of the next
// tile.  One statement reads the B fragments B[k = r0 + 0..7][n = 16*dt + l16]
// of four d tiles: a0..a3 are the LDS addresses of rows r0..r0+3 (lane's row
// r0 + l16/4, its 8 bytes of chunk pair 2*dt), LO the byte offset added for
// r0 inside the tile, HI that of rows r0+4..r0+7.
template <int LO, int HI>
__device__ __forceinline__ void dkv_tr_read4(shortx8 (&b)[4], unsigned a0, unsigned a1,
                                             unsigned a2, unsigned a3) {
  shortx4 l0, h0, l1, h1, l2, h2, l3, h3;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8 offset:%12\n\t"
      "ds_read_b64_tr_b16 %1, %8 offset:%13\n\t"
      "ds_read_b64_tr_b16 %2, %9 offset:%12\n\t"
      "ds_read_b64_tr_b16 %3, %9 offset:%13\n\t"
      "ds_read_b64_tr_b16 %4, %10 offset:%12\n\t"
      "ds_read_b64_tr_b16 %5, %10 offset:%13\n\t"
      "ds_read_b64_tr_b16 %6, %11 offset:%12\n\t"
      "ds_read_b64_tr_b16 %7, %11 offset:%13\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(l0), "=&v"(h0), "=&v"(l1), "=&v"(h1), "=&v"(l2), "=&v"(h2), "=&v"(l3), "=&v"(h3)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "n"(LO), "n"(HI)
      : "memory");
  b[0] = __builtin_shufflevector(l0, h0, 0, 1, 2, 3, 4, 5, 6, 7);
  b[1] = __builtin_shufflevector(l1, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  b[2] = __builtin_shufflevector(l2, h2, 0, 1, 2, 3, 4, 5, 6, 7);
  b[3] = __builtin_shufflevector(l3, h3, 0, 1, 2, 3, 4, 5, 6, 7);
}

// per-wave P^T / dS^T image [64 q][16 kv], 32-byte rows: byte offset of kv
// rows 4*slot..4*slot+3 of q column `q`.  Bit 2 of the row is flipped on odd
// 8-row groups so the two 16-lane groups of a transposed read use opposite
// halves of the bank row; the slot XOR spreads the 16 lanes of a packed
// 8-byte store over all 32 store banks.
__device__ __forceinline__ unsigned dkv_p_off(unsigned q, unsigned slot) {
  return ((q ^ ((q >> 1) & 4u)) << 5) + ((slot ^ ((q >> 2) & 3u)) << 3);
}

// both A fragments A[m = l16][k = 32*kk + 8*lg + 0..7] of the wave image,
// after the wave's own stores to it have landed.  a_lo / a_hi: addresses of
// the lane's row in rows 8*lg+{0..3} / 8*lg+{4..7}; k-step 1 is 32 rows on.
__device__ __forceinline__ void dkv_tr_read_pa(shortx8 (&pa)[2], unsigned a_lo, unsigned a_hi) {
  shortx4 l0, h0, l1, h1;
  asm volatile(
      "s_waitcnt lgkmcnt(0)\n\t"
      "ds_read_b64_tr_b16 %0, %4\n\t"
      "ds_read_b64_tr_b16 %1, %5\n\t"
      "ds_read_b64_tr_b16 %2, %4 offset:1024\n\t"
      "ds_read_b64_tr_b16 %3, %5 offset:1024\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(l0), "=&v"(h0), "=&v"(l1), "=&v"(h1)
      : "v"(a_lo), "v"(a_hi)
      : "memory");
  pa[0] = __builtin_shufflevector(l0, h0, 0, 1, 2, 3, 4, 5, 6, 7);
  pa[1] = __builtin_shufflevector(l1, h1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// acc[dt] += A * B[k = r0 + 0..7][n = 16*dt + l16] over all d tiles, B by
// transposed reads four d tiles at a time.  bt_a[dt]: the lane's address for
// rows 0..3 of buffer 0's Q tile; OFF: byte offset of the tile and of r0 in
// it; boff: byte offset of the buffer.
template <int D, int OFF>
__device__ __forceinline__ void dkv_mma_tr(floatx4* acc, shortx8 a, const unsigned* bt_a,
                                           unsigned boff) {
#pragma unroll
  for (int g = 0; g < D / 64; ++g) {
    shortx8 b[4];
    dkv_tr_read4<OFF, OFF + 4 * D * 2>(b, boff + bt_a[4 * g], boff + bt_a[4 * g + 1],
                                       boff + bt_a[4 * g + 2], boff + bt_a[4 * g + 3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[4 * g + i] = mfma_bf16(a, b[i], acc[4 * g + i]);
  }
}

// GQA: grid.x = b * hkv * (rep / G); the block streams tiles q_start..Sq of q
// head h0, then of h0 + 1, ... h0 + G - 1 through the same two buffers: the
// pipeline is not drained at a head boundary and the buffer parity runs on;
// q0 wraps to q_start and the q / dO / lse bases advance by one head.  rep, G
// and ws are read by the GQA instantiations only.
template <int D, bool CAUSAL, bool GQA>
__launch_bounds__(512)
__global__ void fa_bwd_dkv_kernel(const short* __restrict__ dog, const short* __restrict__ qg,
                                  const short* __restrict__ kg, const short* __restrict__ vg,
                                  const float* __restrict__ lseg, const float* __restrict__ deltag,
                                  short* __restrict__ dkg, short* __restrict__ dvg,
                                  int B, int H, int Sq, int Skv, float scale,
                                  long long q_sb, long long q_sh, long long q_ss,
                                  long long k_sb, long long k_sh, long long k_ss,
                                  long long do_sb, long long do_sh, long long do_ss,
                                  long long dk_sb, long long dk_sh, long long dk_ss,
                                  int rep, int G, float* __restrict__ ws) {
  constexpr int NW = 8;               // waves; block owns NW*16 kv rows
  constexpr int NT = NW * 64;
  constexpr int KVEXT = NW * 16;
  constexpr int QB = 64;
  constexpr int NKK = D / 32;
  constexpr int NDT = D / 16;
  constexpr int TILE = QB * D * 2;           // bytes of one [64][D] tile
  constexpr int NIT = QB * D / (NT * 8);     // DMA instructions per tile
  constexpr int PW = 16 * QB * 2;            // bytes of one wave's P/dS image
  // one array (a second __shared__ object beside a DMA target can cost a
  // vmcnt(0) per LDS read): two {Q, dO} buffers, then the per-wave images
  __shared__ __attribute__((aligned(16))) char lds[4 * TILE + NW * PW];

  const int kvblk = blockIdx.y;     // slow dim; kv0=0 (longest) first
  const int bh = blockIdx.x;
  const int kv0 = kvblk * KVEXT;
  int b = bh / H, h = bh % H;       // h: first q head of the stream
  int hk = h;                       // kv head
  if constexpr (GQA) {
    const int parts = rep / G, bk = bh / parts, hkv = H / rep;
    b = bk / hkv; hk = bk % hkv;
    h = hk * rep + (bh % parts) * G;
  }
  // q, dO and lse / delta bases of the tile that is staged next
  long long qbase = (long long)b * q_sb + (long long)h * q_sh;
  long long dobase = (long long)b * do_sb + (long long)h * do_sh;
  const long long kvbase = (long long)b * k_sb + (long long)hk * k_sh;
  const long long dkbase = (long long)b * dk_sb + (long long)hk * dk_sh;
  // GQA = false keeps bh * Sq: (b * H + h) * Sq is equal but reorders the
  // scalar prologue of the hkv == h kernel
  long long lse_base = GQA ? ((long long)b * H + h) * Sq : ((long long)bh) * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wq = tid >> 6;
  const int l16 = lane & 15;
  const int lg = lane >> 4;

  // K,V fragments (A-layout rows = kv)
  shortx8 kf[NKK], vf[NKK];
  {
    int row = kv0 + wq * 16 + l16;
    bool ok = row < Skv;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      if (ok) {
        kf[kk] = *reinterpret_cast<const shortx8*>(kg + kvbase + (long long)row * k_ss + kk * 32 + lg * 8);
        vf[kk] = *reinterpret_cast<const shortx8*>(vg + kvbase + (long long)row * k_ss + kk * 32 + lg * 8);
      } else {
        for (int i = 0; i < 8; ++i) { kf[kk][i] = 0; vf[kk][i] = 0; }
      }
    }
  }

  floatx4 dk_acc[NDT], dv_acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    dk_acc[dt] = {0.f, 0.f, 0.f, 0.f};
    dv_acc[dt] = {0.f, 0.f, 0.f, 0.f};
  }

  const int q_start = CAUSAL ? (kv0 / QB) * QB : 0;

  // DMA staging map: lane `tid` of instruction `it` fills 16 LDS bytes at
  // it*NT*16 + tid*16 (the DMA target is lane-linear), i.e. chunk position
  // col/8 of row n_row; the chunk that belongs there is position ^ swz(row)
  int n_row[NIT], n_colp[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    int flat = it * NT * 8 + tid * 8;
    int row = flat / D, col = flat % D;
    n_row[it] = row;
    n_colp[it] = col ^ (int)(dkv_swz<D>(row) << 3);
  }

  // stage the Q tile at q0 into qbuf and the dO tile into qbuf + TILE: DMA
  // for a whole tile, zero-padded ordinary stores for the tail tile
  auto stage = [&](int q0, char* qbuf) {
    if (q0 + QB <= Sq) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const short* qsrc = qg + qbase + (long long)(q0 + n_row[it]) * q_ss + n_colp[it];
        const short* dsrc = dog + dobase + (long long)(q0 + n_row[it]) * do_ss + n_colp[it];
        char* dst = qbuf + it * NT * 16 + (tid >> 6) * 64 * 16;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)qsrc,
            (__attribute__((address_space(3))) unsigned int*)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)dsrc,
            (__attribute__((address_space(3))) unsigned int*)(dst + TILE), 16, 0, 0);
      }
    } else {
      constexpr int elems = QB * D;
      for (int flat = tid * 8; flat < elems; flat += NT * 8) {
        int row = flat / D, col = flat % D;
        shortx8 qv, dv;
        if (q0 + row < Sq) {
          qv = *reinterpret_cast<const shortx8*>(qg + qbase + (long long)(q0 + row) * q_ss + col);
          dv = *reinterpret_cast<const shortx8*>(dog + dobase + (long long)(q0 + row) * do_ss + col);
        } else {
          for (int i = 0; i < 8; ++i) { qv[i] = 0; dv[i] = 0; }
        }
        const unsigned o = dkv_off<D>(row, col >> 3);
        *reinterpret_cast<shortx8*>(qbuf + o) = qv;
        *reinterpret_cast<shortx8*>(qbuf + TILE + o) = dv;
      }
    }
  };
  // per-lane lse/delta of the 4 q-subtiles (indexed by C-col = q)
  auto load_stats = [&](int q0, float* lse_o, float* delta_o) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      int q_abs = q0 + nt * 16 + l16;
      lse_o[nt] = (q_abs < Sq) ? lseg[lse_base + q_abs] : INFINITY;
      delta_o[nt] = (q_abs < Sq) ? deltag[lse_base + q_abs] : 0.f;
    }
  };

  char* const pw = lds + 4 * TILE + wq * PW;
  // LDS addresses of the lane's rows for the transposed reads
  const unsigned lds_a = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  const unsigned tr_q = l16 >> 2, tr_p = l16 & 3;
  unsigned bt_a[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
    bt_a[dt] = lds_a + dkv_off<D>(8 * lg + tr_q, 2 * dt + (tr_p >> 1)) + ((tr_p & 1) << 3);
  const unsigned pa_lo = lds_a + 4 * TILE + wq * PW + dkv_p_off(8 * lg + tr_q, tr_p);
  const unsigned pa_hi = lds_a + 4 * TILE + wq * PW + dkv_p_off(8 * lg + 4 + tr_q, tr_p);
  float lse_n[4], delta_n[4];
  if (q_start < Sq) {
    stage(q_start, lds);
    load_stats(q_start, lse_n, delta_n);
  }
  int cur = 0;
  int hleft = GQA ? G - 1 : 0;      // q heads of the stream after the staged one
  for (int q0 = q_start, qn; q0 < Sq; q0 = qn) {
    // Tile q0 was issued one tile ago (or in the prologue) and nothing newer
    // is in flight, so the counted wait is vmcnt(0).  The one barrier per
    // tile then says both "tile q0 has landed for every wave" and "every
    // wave is done reading the tile before", which frees the other buffer.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned boff = cur * (2 * TILE);
    const char* q_t = lds + boff;
    float lse_v[4], delta_v[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) { lse_v[nt] = lse_n[nt]; delta_v[nt] = delta_n[nt]; }
    qn = q0 + QB;
    if constexpr (GQA) {
      if (qn >= Sq && hleft > 0) {   // head boundary: the next head's first tile
        --hleft;
        qn = q_start;
        qbase += q_sh; dobase += do_sh; lse_base += Sq;
      }
    }
    if (qn < Sq) {
      stage(qn, lds + (cur ^ 1) * (2 * TILE));
      load_stats(qn, lse_n, delta_n);
    }
    cur ^= 1;
    const char* do_t = q_t + TILE;

    // S^T = K Q^T ; P^T = exp(S^T*scale - lse[q])
    floatx4 pt[4];
    const int kv_abs0 = kv0 + wq * 16 + lg * 4;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      floatx4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        shortx8 qfr = *reinterpret_cast<const shortx8*>(
            q_t + dkv_off<D>(nt * 16 + l16, kk * 4 + lg));
        st = mfma_bf16(kf[kk], qfr, st);
      }
      const int q_abs = q0 + nt * 16 + l16;
      const bool bnd = (q0 + QB > Sq) || (kv0 + KVEXT > Skv) ||
                       (CAUSAL && q0 < kv0 + KVEXT);
      if (bnd) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int kv_abs = kv_abs0 + r;
          float p = __expf(st[r] * scale - lse_v[nt]);
          if (q_abs >= Sq || kv_abs >= Skv || (CAUSAL && kv_abs > q_abs)) p = 0.f;
          pt[nt][r] = p;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pt[nt][r] = __expf(st[r] * scale - lse_v[nt]);
      }
    }

    // P^T (then dS^T) to the wave's [q][kv] image: a lane holds kv rows
    // 4*lg..4*lg+3 of q column nt*16+l16, one packed 8-byte store per C tile
    shortx8 pa[2];
    auto put_get = [&]() {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        shortx4 v = {f2bf(pt[nt][0]), f2bf(pt[nt][1]), f2bf(pt[nt][2]), f2bf(pt[nt][3])};
        *reinterpret_cast<shortx4*>(pw + dkv_p_off(nt * 16 + l16, lg)) = v;
      }
      dkv_tr_read_pa(pa, pa_lo, pa_hi);
    };
    put_get();

    // dV += P^T dO   (A = P^T from the wave image, B = dO by transposed reads)
    dkv_mma_tr<D, TILE>(dv_acc, pa[0], bt_a, boff);
    dkv_mma_tr<D, TILE + 32 * D * 2>(dv_acc, pa[1], bt_a, boff);

    // dP^T = V dO^T
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      floatx4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        shortx8 bfr = *reinterpret_cast<const shortx8*>(
            do_t + dkv_off<D>(nt * 16 + l16, kk * 4 + lg));
        dp = mfma_bf16(vf[kk], bfr, dp);
      }
      // dS^T = P^T * (dP^T - delta[q]) * scale
#pragma unroll
      for (int r = 0; r < 4; ++r)
        pt[nt][r] = pt[nt][r] * (dp[r] - delta_v[nt]) * scale;
    }
    put_get();   // the reads of P^T ended inside the first put_get

    // dK += dS^T Q  (B = Q by transposed reads)
    dkv_mma_tr<D, 0>(dk_acc, pa[0], bt_a, boff);
    dkv_mma_tr<D, 32 * D * 2>(dk_acc, pa[1], bt_a, boff);
  }

  // write dK, dV
  if constexpr (GQA) {
    if (G != rep) {   // fp32 partials [grid.x, Skv, D]: dK, then dV
      float* wk = ws + (long long)bh * Skv * D;
      float* wv = wk + (long long)gridDim.x * Skv * D;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = kv0 + wq * 16 + lg * 4 + r;
        if (row >= Skv) continue;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          wk[(long long)row * D + dt * 16 + l16] = dk_acc[dt][r];
          wv[(long long)row * D + dt * 16 + l16] = dv_acc[dt][r];
        }
      }
      return;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int row = kv0 + wq * 16 + lg * 4 + r;
    if (row >= Skv) continue;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      dkg[dkbase + (long long)row * dk_ss + dt * 16 + l16] = f2bf(dk_acc[dt][r]);
      dvg[dkbase + (long long)row * dk_ss + dt * 16 + l16] = f2bf(dv_acc[dt][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// backward dQ, 32x32 variant: same swapped layout as the forward -- S^T and
// dP^T put the q-COLUMN in each lane (per-lane lse/delta, no broadcasts),
// and the dS A-fragments for dQ += dS.K are assembled with the identical
// static-pack + permlane32_swap exchange (no LDS round trip).
// K and V land once per tile, by DMA, in the natural [64 kv][D] image of the
// forward (fa_common.h, fa_kv_off).  The K image feeds S^T by ds_read_b128
// rows and dQ += dS K by ds_read_b64_tr_b16, so K is read once from global
// and no transposed copy is built; V takes row reads only.  Two {K, V}
// buffers, tile t+1 in flight under tile t's math, one barrier per tile.
// Every MFMA gets the operands, in the k order, of the kernel this replaces
// (K^T by scalar writes, one buffer), so dQ is bit-identical to it.
// Measured, B12 H32 S2048 D128 causal: 1369 -> 877 us per call in the
// flagship trace, SQ_LDS_BANK_CONFLICT 1.4e8 -> 0, 256 VGPR + 12 B scratch ->
// 248 VGPR and none (docs/KERNELS.md, "forward and dQ").
// ---------------------------------------------------------------------------
// GQA: K / V come from head h / rep (the forward's head map); rep is read
// by the GQA instantiations only.
template <int D, bool CAUSAL, bool MASKED, bool DROPOUT, bool VARLEN, bool GQA>
__launch_bounds__(256, 2)
__global__ void fa_bwd_dq32_kernel(const short* __restrict__ dog, const short* __restrict__ qg,
                                   const short* __restrict__ kg, const short* __restrict__ vg,
                                   const float* __restrict__ lseg, const float* __restrict__ deltag,
                                   short* __restrict__ dqg, int B, int H, int Sq, int Skv,
                                   float scale,
                                   long long q_sb, long long q_sh, long long q_ss,
                                   long long k_sb, long long k_sh, long long k_ss,
                                   long long do_sb, long long do_sh, long long do_ss,
                                   long long dq_sb, long long dq_sh, long long dq_ss,
                                   const short* __restrict__ maskg, long long m_sb,
                                   long long m_sh, long long m_sq,
                                   float pdrop, unsigned long long rseed,
                                   unsigned long long roffset,
                                   const int* __restrict__ cu_q,
                                   const int* __restrict__ cu_k,
                                   const int* __restrict__ bmap, int rep) {
  constexpr int NW = 4;
  constexpr int NT = NW * 64;
  constexpr int QB = NW * 32;       // 128 q rows / block
  constexpr int KB = 64;
  constexpr int NKS = D / 16;
  constexpr int NDT = D / 32;
  constexpr int TILE = KB * D * 2;  // bytes of one [64][D] tile
  // one array: two {K, V} buffers (fa_common.h, fa_stage_kv)
  __shared__ __attribute__((aligned(16))) char lds[4 * TILE];

  const int qblk = blockIdx.y;      // slow dim: global longest-first causal order
  const int bh = blockIdx.x;
  int b = bh / H, h = bh % H;
  int q0, Sq_e = Sq, Skv_e = Skv, cdelta = 0, qglob0 = 0;
  long long qbase, dobase, dqbase, kvbase;
  if (VARLEN) {
    b = 0; h = bh;
    const int seq = bmap[2 * qblk];
    q0 = bmap[2 * qblk + 1];
    const int qs0 = cu_q[seq], ks0 = cu_k[seq];
    Sq_e = cu_q[seq + 1] - qs0;
    Skv_e = cu_k[seq + 1] - ks0;
    cdelta = Skv_e - Sq_e;
    qglob0 = qs0;
    qbase = (long long)qs0 * q_ss + (long long)h * q_sh;
    dobase = (long long)qs0 * do_ss + (long long)h * do_sh;
    dqbase = (long long)qs0 * dq_ss + (long long)h * dq_sh;
    kvbase = (long long)ks0 * k_ss + (long long)(GQA ? h / rep : h) * k_sh;
  } else {
    q0 = (CAUSAL ? ((int)gridDim.y - 1 - qblk) : qblk) * QB;   // longest-first
    qbase = (long long)b * q_sb + (long long)h * q_sh;
    dobase = (long long)b * do_sb + (long long)h * do_sh;
    dqbase = (long long)b * dq_sb + (long long)h * dq_sh;
    kvbase = (long long)b * k_sb + (long long)(GQA ? h / rep : h) * k_sh;
  }
  const long long lse_base = ((long long)bh) * Sq + qglob0;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wq = tid >> 6;
  const int l32 = lane & 31;
  const int hi = lane >> 5;
  const int q0w = q0 + wq * 32;

  // Q and dO as B-fragments (lane holds the q column l32); Q pre-scaled
  // by the softmax scale so the exp loop skips a per-element mul
  shortx8 qf[NKS], dof[NKS];
  {
    int row = q0w + l32;
    bool ok = row < Sq_e;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      if (ok) {
        shortx8 raw = *reinterpret_cast<const shortx8*>(
            qg + qbase + (long long)row * q_ss + ks * 16 + hi * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) qf[ks][i] = f2bf(bf2f(raw[i]) * scale);
        dof[ks] = *reinterpret_cast<const shortx8*>(
            dog + dobase + (long long)row * do_ss + ks * 16 + hi * 8);
      } else {
        for (int i = 0; i < 8; ++i) { qf[ks][i] = 0; dof[ks][i] = 0; }
      }
    }
  }
  const int q_abs = q0w + l32;
  const float lse_v = (q_abs < Sq_e) ? lseg[lse_base + q_abs] : 1e30f;
  const float delta_v = (q_abs < Sq_e) ? deltag[lse_base + q_abs] : 0.f;

  floatx16 dq_acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;

  // LDS addresses of the lane's rows for the transposed reads of K
  const unsigned lds_a = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  unsigned tr_a[2][NDT];   // even, odd k-steps
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    tr_a[0][dt] = fa_tr_addr<D>(lds_a, lane, dt, 0);
    tr_a[1][dt] = fa_tr_addr<D>(lds_a, lane, dt, 16);
  }

  const int kv_end = CAUSAL ? min(Skv_e, q0 + QB + cdelta) : Skv_e;
  if (kv_end > 0) fa_stage_kv<D, NT>(lds, kg, vg, kvbase, k_ss, 0, Skv_e, tid);
  int cur = 0;
  for (int kv0 = 0; kv0 < kv_end; kv0 += KB) {
    // Tile kv0 was issued one tile ago (or in the prologue) and nothing newer
    // is in flight, so the counted wait is vmcnt(0).  The one barrier per
    // tile says both "tile kv0 has landed for every wave" and "every wave is
    // done reading tile kv0-KB", which frees the other buffer.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned boff = cur * (2 * TILE);
    const char* k_t = lds + boff;
    const char* v_t = k_t + TILE;
    if (kv0 + KB < kv_end)
      fa_stage_kv<D, NT>(lds + (cur ^ 1) * (2 * TILE), kg, vg, kvbase, k_ss, kv0 + KB, Skv_e, tid);
    cur ^= 1;

    // ---- S^T = K Q^T and dP^T = V dO^T ------------------------------------
    floatx16 st[2], dp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { st[t][r] = 0.f; dp[t][r] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        shortx8 kf = *reinterpret_cast<const shortx8*>(
            k_t + fa_kv_off<D>(t * 32 + l32, ks * 2 + hi));
        st[t] = mfma32_bf16(kf, qf[ks], st[t]);
        shortx8 vf = *reinterpret_cast<const shortx8*>(
            v_t + fa_kv_off<D>(t * 32 + l32, ks * 2 + hi));
        dp[t] = mfma32_bf16(vf, dof[ks], dp[t]);
      }
    }

    // ---- dS^T = P^T (dP^T o dropout - delta) * scale ----------------------
    if (MASKED && q_abs < Sq_e) {
      const short* mrow = maskg + (long long)b * m_sb + (long long)h * m_sh
                        + (long long)q_abs * m_sq;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          long long kvb = kv0 + 32 * t + 8 * g + 4 * hi;
          if (kvb + 3 < Skv_e) {
            shortx4 mv = *reinterpret_cast<const shortx4*>(mrow + kvb);
#pragma unroll
            for (int j = 0; j < 4; ++j) st[t][4 * g + j] += bf2f(mv[j]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (kvb + j < Skv_e) st[t][4 * g + j] += bf2f(mrow[kvb + j]);
          }
        }
    }
    const bool bnd = (kv0 + KB > Skv_e) || (CAUSAL && kv0 + KB > q_abs + cdelta);
    const float inv_keep = DROPOUT ? 1.f / (1.f - pdrop) : 1.f;
    const unsigned thr24 = DROPOUT ? (unsigned)(pdrop * 16777216.f) : 0u;
    const long long bh_ll = (long long)b * H + h;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (DROPOUT) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          long long kvb = kv0 + 32 * t + 8 * g + 4 * hi;
          long long elem = (bh_ll * Sq + (q_abs + qglob0)) * (long long)Skv + kvb;
          uintx4 rv = philox10(rseed, roffset + (unsigned long long)(elem >> 2));
#pragma unroll
          for (int j = 0; j < 4; ++j)
            dp[t][4 * g + j] = ((rv[j] >> 8) >= thr24)
                                   ? dp[t][4 * g + j] * inv_keep : 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p = __expf(st[t][r] - lse_v);   // Q pre-scaled at load
        if (bnd) {
          int kv_abs = kv0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (kv_abs >= Skv_e || (CAUSAL && kv_abs > q_abs + cdelta)) p = 0.f;
        }
        st[t][r] = p * (dp[t][r] - delta_v) * scale;
      }
    }

    // ---- dQ += dS K (A-frags via static packs + permlane exchange) --------
    // one k-step of 16 kv rows; KS is a type so the offsets of the
    // transposed reads are immediates
    auto dq_step = [&](auto KS) {
      constexpr int ks = decltype(KS)::value;
      constexpr int t = ks >> 1;
      constexpr int kp = ks & 1;
      constexpr int b0 = 8 * kp;
      int P0 = pack_bf2(st[t][b0 + 0], st[t][b0 + 1]);
      int P1 = pack_bf2(st[t][b0 + 2], st[t][b0 + 3]);
      int P2 = pack_bf2(st[t][b0 + 4], st[t][b0 + 5]);
      int P3 = pack_bf2(st[t][b0 + 6], st[t][b0 + 7]);
      int O1 = hi ? P2 : P0;
      int O2 = hi ? P3 : P1;
      int S1 = hi ? P0 : P2;
      int S2 = hi ? P1 : P3;
      intx2 ra = __builtin_amdgcn_permlane32_swap(S1, S2, false, false);
      intx2 rb = __builtin_amdgcn_permlane32_swap(S2, S1, false, false);
      int X1 = hi ? rb[0] : ra[1];
      int X2 = hi ? ra[0] : rb[1];
      intx4 paw;
      paw[0] = hi ? X1 : O1;
      paw[1] = hi ? X2 : O2;
      paw[2] = hi ? O1 : X1;
      paw[3] = hi ? O2 : X2;
      shortx8 pa = *reinterpret_cast<shortx8*>(&paw);
      // B[k = 16*ks + 8*hi + 0..7][n = 32*dt + l32] of K, by transposed reads
      // of the image that fed S^T by rows
      shortx8 bf[NDT];
      unsigned ka[NDT];
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) ka[dt] = boff + tr_a[kp][dt];
      fa_tr_read<D, ks * 16 * D * 2>(bf, ka);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) dq_acc[dt] = mfma32_bf16(pa, bf[dt], dq_acc[dt]);
    };
    dq_step(std::integral_constant<int, 0>{});
    dq_step(std::integral_constant<int, 1>{});
    dq_step(std::integral_constant<int, 2>{});
    dq_step(std::integral_constant<int, 3>{});
  }

  // ---- epilogue -----------------------------------------------------------
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int rq = (r & 3) + 8 * (r >> 2) + 4 * hi;
    int row = q0w + rq;
    if (row >= Sq_e) continue;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      dqg[dqbase + (long long)row * dq_ss + dt * 32 + l32] = f2bf(dq_acc[dt][r]);
  }
}

// ---------------------------------------------------------------------------
// backward dV / dK, 32x32 split variant (v3).
//
// Orientation: P = mfma(Q, K) and dP = mfma(dO, V) put the kv column in
// the LANE dim, so P / dS feed dV^T = dO^T P and dK^T = Q^T dS as
// B-fragments via the forward's static-pack + permlane32_swap exchange --
// no lane<->reg transpose, no LDS round trip (the v1 split's failure).
// Split into dV and dK kernels so each fits 2 waves/SIMD (the combined
// variant needs 128 accumulator VGPRs and runs at occupancy 1, measured
// slower than the 16x16 kernel).  Q / dO A-fragments are read straight
// from global (all 4 waves read the same rows -> L2-served); only the
// transposed operand (dO^T or Q^T) is staged in LDS, double-buffered.
// Outputs are accumulated transposed and written as packed 8 B stores.
// ---------------------------------------------------------------------------
// Keeps its scalar arguments and its own prologue: its mask + dropout dK
// instantiations sit at the 256-VGPR limit, and with FaArgs and fa_block
// their scratch size moves by a few bytes.
// GQA: as fa_bwd_dkv_kernel, grid.x = b * hkv * (rep / G) and one tile stream
// over the G q heads of the block; the dropout element index follows the q
// head of the tile.  rep, G and ws (this launch's fp32 partials
// [grid.x, Skv, D]) are read by the GQA instantiations only.
template <int D, bool CAUSAL, bool IS_DK, bool MASKED, bool DROPOUT, bool VARLEN, bool GQA>
__launch_bounds__(256, 2)
__global__ void fa_bwd_dkv32_kernel(const short* __restrict__ dog, const short* __restrict__ qg,
                                    const short* __restrict__ kg, const short* __restrict__ vg,
                                    const float* __restrict__ lseg, const float* __restrict__ deltag,
                                    short* __restrict__ outg,
                                    int B, int H, int Sq, int Skv, float scale,
                                    long long q_sb, long long q_sh, long long q_ss,
                                    long long k_sb, long long k_sh, long long k_ss,
                                    long long do_sb, long long do_sh, long long do_ss,
                                    long long dk_sb, long long dk_sh, long long dk_ss,
                                    const short* __restrict__ maskg, long long m_sb,
                                    long long m_sh, long long m_sq,
                                    float pdrop, unsigned long long rseed,
                                    unsigned long long roffset,
                                    const int* __restrict__ cu_q,
                                    const int* __restrict__ cu_k,
                                    const int* __restrict__ bmap,
                                    int rep, int G, float* __restrict__ ws) {
  constexpr int NW = 4;
  constexpr int NT = NW * 64;
  constexpr int KVB = NW * 32;     // 128 kv rows / block
  constexpr int QT = 32;           // q tile (one 32-q mfma tile)
  constexpr int NKS = D / 16;
  constexpr int NDT = D / 32;
  constexpr unsigned TR_RS = 64 * 2;  // transposed rows padded to 64 cols
  // transposed operand (dO^T for dV, Q^T for dK): rows = d (128), padded to
  // 64 bf16 columns so lds_off32's 8-row XOR swizzle stays in-row
  __shared__ char t_lds[2][D * 64 * 2];
  __shared__ float stat_s[2][2 * QT];  // [lse | delta]

  const int kvblk = blockIdx.y;     // slow dim; kv0=0 (longest) dispatches first
  const int bh = blockIdx.x;
  int b = bh / H, h = bh % H;       // h: q head of the current tile
  int hk = h;                       // kv head
  if constexpr (GQA) {              // varlen: b = 0 and H = h, so one map serves both
    const int parts = rep / G, bk = bh / parts, hkv = H / rep;
    b = bk / hkv; hk = bk % hkv;
    h = hk * rep + (bh % parts) * G;
  }
  int kv0, Sq_e = Sq, Skv_e = Skv, cdelta = 0, qglob0 = 0, kglob0 = 0;
  long long qbase_c, dobase_c, kvbase, outbase;   // _c: of the current tile's head
  if (VARLEN) {
    if constexpr (!GQA) { b = 0; h = bh; hk = h; }
    const int seq = bmap[2 * kvblk];
    kv0 = bmap[2 * kvblk + 1];
    const int qs0 = cu_q[seq], ks0 = cu_k[seq];
    Sq_e = cu_q[seq + 1] - qs0;
    Skv_e = cu_k[seq + 1] - ks0;
    cdelta = Skv_e - Sq_e;
    qglob0 = qs0;
    kglob0 = ks0;
    qbase_c = (long long)qs0 * q_ss + (long long)h * q_sh;
    dobase_c = (long long)qs0 * do_ss + (long long)h * do_sh;
    kvbase = (long long)ks0 * k_ss + (long long)hk * k_sh;
    outbase = (long long)ks0 * dk_ss + (long long)hk * dk_sh;
  } else {
    kv0 = kvblk * KVB;
    qbase_c = (long long)b * q_sb + (long long)h * q_sh;
    dobase_c = (long long)b * do_sb + (long long)h * do_sh;
    kvbase = (long long)b * k_sb + (long long)hk * k_sh;
    outbase = (long long)b * dk_sb + (long long)hk * dk_sh;
  }
  long long lse_base_c = GQA ? ((long long)b * H + h) * Sq + qglob0
                           : ((long long)bh) * Sq + qglob0;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wq = tid >> 6;
  const int l32 = lane & 31;
  const int hi = lane >> 5;
  const int kv0w = kv0 + wq * 32;
  const int kv_lane = kv0w + l32;

  // K (and V for dK) as B-fragments (lane = kv row), loaded once
  shortx8 kf[NKS], vf[IS_DK ? NKS : 1];
  {
    bool ok = kv_lane < Skv_e;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      if (ok) {
        kf[ks] = *reinterpret_cast<const shortx8*>(
            kg + kvbase + (long long)kv_lane * k_ss + ks * 16 + hi * 8);
        if (IS_DK)
          vf[ks] = *reinterpret_cast<const shortx8*>(
              vg + kvbase + (long long)kv_lane * k_ss + ks * 16 + hi * 8);
      } else {
        for (int i = 0; i < 8; ++i) { kf[ks][i] = 0; if (IS_DK) vf[ks][i] = 0; }
      }
    }
  }

  floatx16 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;

  // stage the transposed operand tile (rotated scalar writes) + stats of
  // the head `hadv` (0 or 1) after the current one
  auto stage = [&](int buf, int q0, int hadv) {
    const long long lse_base = lse_base_c + (GQA ? (long long)hadv * Sq : 0);
    const long long qbase = qbase_c + (GQA ? hadv * q_sh : 0);
    const long long dobase = dobase_c + (GQA ? hadv * do_sh : 0);
    if (tid < QT) {
      int qa = q0 + tid;
      stat_s[buf][tid] = (qa < Sq_e) ? lseg[lse_base + qa] : 1e30f;
      if (IS_DK)
        stat_s[buf][QT + tid] = (qa < Sq_e) ? deltag[lse_base + qa] : 0.f;
    }
    const int rot = tid & 7;
    for (int flat = tid * 8; flat < QT * D; flat += NT * 8) {
      int row = flat / D, col = flat % D;   // row = q, col = d
      shortx8 v;
      if (q0 + row < Sq_e) {
        const short* src = IS_DK
            ? qg + qbase + (long long)(q0 + row) * q_ss + col
            : dog + dobase + (long long)(q0 + row) * do_ss + col;
        v = *reinterpret_cast<const shortx8*>(src);
      } else {
        for (int i = 0; i < 8; ++i) v[i] = 0;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int i = (j + rot) & 7;
        *reinterpret_cast<short*>(t_lds[buf] + lds_off32(col + i, row * 2, TR_RS)) = v[i];
      }
    }
  };

  const int q_start = CAUSAL ? (max(0, kv0 - cdelta) / QT) * QT : 0;
  stage(0, q_start, 0);
  __syncthreads();
  int cur = 0;
  int hleft = GQA ? G - 1 : 0;      // q heads of the stream after the current one
  for (int q0 = q_start, qn; q0 < Sq_e; q0 = qn) {
    const long long qbase = qbase_c, dobase = dobase_c;
    qn = q0 + QT;
    int hadv = 0;
    if constexpr (GQA) {
      if (qn >= Sq_e && hleft > 0) {   // head boundary: the next head's first tile
        --hleft;
        qn = q_start;
        hadv = 1;
      }
    }
    if (qn < Sq_e) stage(cur ^ 1, qn, hadv);

    // Q (and dO for dK) A-fragments straight from global: lane = q row
    const int q_lane = q0 + l32;
    const bool qok = q_lane < Sq_e;
    floatx16 st, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      shortx8 qa;
      if (qok)
        qa = *reinterpret_cast<const shortx8*>(
            qg + qbase + (long long)q_lane * q_ss + ks * 16 + hi * 8);
      else
        for (int i = 0; i < 8; ++i) qa[i] = 0;
      st = mfma32_bf16(qa, kf[ks], st);
      if (IS_DK) {
        shortx8 da;
        if (qok)
          da = *reinterpret_cast<const shortx8*>(
              dog + dobase + (long long)q_lane * do_ss + ks * 16 + hi * 8);
        else
          for (int i = 0; i < 8; ++i) da[i] = 0;
        dp = mfma32_bf16(da, vf[ks], dp);
      }
    }

    // per-reg q stats + exp/mask.  For dV, P = exp(S*scale - lse[q]); for
    // dK additionally dS = P (dP - delta[q]) * scale -- but P needs lse
    // there too, so dK stages BOTH: lse comes from a second pass of
    // broadcast loads straight from global (L2-hot after the dV kernel).
    const bool bnd = (q0 + QT > Sq_e) || (kv0w + 32 > Skv_e) ||
                     (CAUSAL && kv0w + 32 > q0 + cdelta);
    const float inv_keep = DROPOUT ? 1.f / (1.f - pdrop) : 1.f;
    const unsigned thr24 = DROPOUT ? (unsigned)(pdrop * 16777216.f) : 0u;
    const long long bh_ll = (long long)b * H + h;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rq = (r & 3) + 8 * (r >> 2) + 4 * hi;
      const int q_abs = q0 + rq;
      float sc = st[r] * scale;
      if (MASKED && q_abs < Sq_e && kv_lane < Skv_e)
        sc += bf2f(maskg[(long long)b * m_sb + (long long)h * m_sh
                         + (long long)q_abs * m_sq + kv_lane]);
      float p = __expf(sc - stat_s[cur][rq]);
      if (bnd) {
        if (q_abs >= Sq_e || kv_lane >= Skv_e ||
            (CAUSAL && kv_lane > q_abs + cdelta)) p = 0.f;
      }
      bool keep = true;
      if (DROPOUT)
        keep = fa_keep(rseed, roffset, bh_ll, Sq, Skv, q_abs + qglob0,
                       kv_lane, thr24);
      if (IS_DK) {
        float dpe = dp[r];
        if (DROPOUT) dpe = keep ? dpe * inv_keep : 0.f;
        st[r] = p * (dpe - stat_s[cur][QT + rq]) * scale;
      } else {
        if (DROPOUT) p = keep ? p * inv_keep : 0.f;
        st[r] = p;
      }
    }

    // ---- acc += (dO^T P) or (Q^T dS): B-frags via pack+permlane ----------
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int b0 = 8 * ks;
      int P0 = pack_bf2(st[b0 + 0], st[b0 + 1]);
      int P1 = pack_bf2(st[b0 + 2], st[b0 + 3]);
      int P2 = pack_bf2(st[b0 + 4], st[b0 + 5]);
      int P3 = pack_bf2(st[b0 + 6], st[b0 + 7]);
      int O1 = hi ? P2 : P0, O2 = hi ? P3 : P1;
      int S1 = hi ? P0 : P2, S2 = hi ? P1 : P3;
      intx2 ra = __builtin_amdgcn_permlane32_swap(S1, S2, false, false);
      intx2 rb = __builtin_amdgcn_permlane32_swap(S2, S1, false, false);
      int X1 = hi ? rb[0] : ra[1], X2 = hi ? ra[0] : rb[1];
      intx4 paw;
      paw[0] = hi ? X1 : O1; paw[1] = hi ? X2 : O2;
      paw[2] = hi ? O1 : X1; paw[3] = hi ? O2 : X2;
      shortx8 frag = *reinterpret_cast<shortx8*>(&paw);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        shortx8 tfr = *reinterpret_cast<const shortx8*>(
            t_lds[cur] + lds_off32(dt * 32 + l32, (ks * 16 + hi * 8) * 2, TR_RS));
        acc[dt] = mfma32_bf16(tfr, frag, acc[dt]);
      }
    }
    __syncthreads();
    cur ^= 1;
    if constexpr (GQA) {
      if (hadv) { ++h; qbase_c += q_sh; dobase_c += do_sh; lse_base_c += Sq; }
    }
  }

  // ---- epilogue: transposed accumulators -> natural rows ------------------
  if constexpr (GQA) {
    if (G != rep) {   // fp32 partials, 16-byte stores
      if (kv_lane < Skv_e) {
        float* wrow = ws + ((long long)bh * Skv + kglob0 + kv_lane) * D;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            floatx4 pv = {acc[dt][g * 4], acc[dt][g * 4 + 1], acc[dt][g * 4 + 2],
                          acc[dt][g * 4 + 3]};
            *reinterpret_cast<floatx4*>(wrow + dt * 32 + 8 * g + 4 * hi) = pv;
          }
      }
      return;
    }
  }
  if (kv_lane < Skv_e) {
    const long long orow = outbase + (long long)kv_lane * dk_ss;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        shortx4 pv;
#pragma unroll
        for (int i = 0; i < 4; ++i) pv[i] = f2bf(acc[dt][g * 4 + i]);
        int d = dt * 32 + 8 * g + 4 * hi;
        *reinterpret_cast<shortx4*>(outg + orow + d) = pv;
      }
  }
}

// ---------------------------------------------------------------------------
// GQA with G < rep: sums the rep/G fp32 partials of each kv head, in the order
// of the q heads, and writes bf16 dK / dV through dk_s.  ws holds
// [nbk * parts, Skv, D] for dK, then the same for dV (nbk = b * hkv); n4 is
// nbk * Skv * D / 4, the 16-byte groups of one output tensor.  Grid-stride,
// 16-byte loads, 8-byte stores, no atomics: the result depends on nothing
// but the partials.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fa_bwd_gqa_reduce_kernel(
    const float* __restrict__ ws, short* __restrict__ dkg, short* __restrict__ dvg,
    int hkv, int parts, int Skv, int D4, long long n4,
    long long dk_sb, long long dk_sh, long long dk_ss) {
  const floatx4* ws4 = reinterpret_cast<const floatx4*>(ws);
  const long long pstride = (long long)Skv * D4;   // one partial, in 16-byte groups
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < 2 * n4;
       i += (long long)gridDim.x * 256) {
    const bool is_dv = i >= n4;
    const long long j = is_dv ? i - n4 : i;
    const int c4 = (int)(j % D4);
    const int row = (int)((j / D4) % Skv);
    const long long bk = j / pstride;
    const floatx4* src = ws4 + (is_dv ? n4 * parts : 0) + (bk * parts) * pstride
                       + (long long)row * D4 + c4;
    floatx4 acc = src[0];
    for (int p = 1; p < parts; ++p) acc += src[p * pstride];
    const shortx4 o = {f2bf(acc[0]), f2bf(acc[1]), f2bf(acc[2]), f2bf(acc[3])};
    short* dst = (is_dv ? dvg : dkg) + (bk / hkv) * dk_sb + (bk % hkv) * dk_sh
               + (long long)row * dk_ss + c4 * 4;
    *reinterpret_cast<shortx4*>(dst) = o;
  }
}

// ---------------------------------------------------------------------------
// host launcher: delta, then dK / dV, then dQ.  Dense without mask and
// dropout takes fa_bwd_dkv_kernel for dK / dV; every other path takes
// fa_bwd_dkv32_kernel, once for dV and once for dK.  The kernels keep scalar
// arguments (see docs/KERNELS.md, launch path); FA_BWD_ARGS spells them out
// once, from the named fields of FaArgs.  hkv != h picks the GQA
// instantiations (dense without mask, varlen); their dK/dV grid is
// b * hkv * (rep / G) wide, and G < rep adds the reduce over a.gqa_ws.
// ---------------------------------------------------------------------------
#define FA_BWD_ARGS(OUT_S)                                                      \
  a.b, a.h, a.sq, a.skv, a.scale, a.q_s.b, a.q_s.h, a.q_s.s,                    \
  a.k_s.b, a.k_s.h, a.k_s.s, a.do_s.b, a.do_s.h, a.do_s.s,                      \
  a.OUT_S.b, a.OUT_S.h, a.OUT_S.s
#define FA_BWD_TAIL(BMAP)                                                       \
  (const short*)a.mask, a.m_s.b, a.m_s.h, a.m_s.s, a.pdrop, a.seed, a.offset,   \
  a.cu_q, a.cu_k, a.BMAP

void flash_attn_bwd(const FaArgs& a, hipStream_t s) {
  const bool varlen = a.cu_q != nullptr;
  flash_attn_bwd_delta(a.dout, a.o, a.delta, a.b, a.h, a.sq, a.dh, a.do_s, a.o_s, s);
  const int rep = a.h / a.hkv;
  const int G = a.gqa_heads > 0 ? a.gqa_heads : rep;   // q heads per dK/dV block
  const dim3 gkv((unsigned)(a.b * (a.h / G)),
                 (unsigned)(varlen ? a.n_kvblocks : cdiv(a.skv, 128)));
  const dim3 gq((unsigned)(a.b * a.h),
                (unsigned)(varlen ? a.n_qblocks : cdiv(a.sq, 128)));
  const short *dout = (const short*)a.dout, *q = (const short*)a.q;
  const short *k = (const short*)a.k, *v = (const short*)a.v;
  const float *lse = a.lse, *delta = a.delta;
  // fp32 partials of one output tensor (G < rep only)
  const long long ws_half = (long long)gkv.x * a.skv * a.dh;
  auto dkv32 = [&](auto dv_kernel, auto dk_kernel) {   // dV, then dK
    hipLaunchKernelGGL(dv_kernel, gkv, dim3(256), 0, s, dout, q, k, v, lse, delta,
                       (short*)a.dv, FA_BWD_ARGS(dk_s), FA_BWD_TAIL(kv_bmap),
                       rep, G, a.gqa_ws + (G != rep ? ws_half : 0));
    hipLaunchKernelGGL(dk_kernel, gkv, dim3(256), 0, s, dout, q, k, v, lse, delta,
                       (short*)a.dk, FA_BWD_ARGS(dk_s), FA_BWD_TAIL(kv_bmap),
                       rep, G, a.gqa_ws);
  };
  auto dq32 = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, gq, dim3(256), 0, s, dout, q, k, v, lse, delta,
                       (short*)a.dq, FA_BWD_ARGS(dq_s), FA_BWD_TAIL(q_bmap), rep);
  };
  fa_dispatch_gqa(a, [&](auto D, auto C, auto M, auto P, auto Q) {
    if constexpr (M() && Q()) {
      // no GQA + mask instantiations: the binding refuses the call
    } else if (!varlen) {
      if constexpr (!M() && !P())
        hipLaunchKernelGGL((fa_bwd_dkv_kernel<D(), C(), Q()>), gkv, dim3(512), 0, s, dout, q, k,
                           v, lse, delta, (short*)a.dk, (short*)a.dv, FA_BWD_ARGS(dk_s),
                           rep, G, a.gqa_ws);
      else
        dkv32(fa_bwd_dkv32_kernel<D(), C(), false, M(), P(), false, Q()>,
              fa_bwd_dkv32_kernel<D(), C(), true, M(), P(), false, Q()>);
      dq32(fa_bwd_dq32_kernel<D(), C(), M(), P(), false, Q()>);
    } else if constexpr (!M()) {   // varlen takes no mask
      dkv32(fa_bwd_dkv32_kernel<D(), C(), false, false, P(), true, Q()>,
            fa_bwd_dkv32_kernel<D(), C(), true, false, P(), true, Q()>);
      dq32(fa_bwd_dq32_kernel<D(), C(), false, P(), true, Q()>);
    }
  });
  if (G != rep) {
    const long long n4 = (long long)a.b * a.hkv * a.skv * a.dh / 4;
    const dim3 gr((unsigned)hmin<long long>(2048LL, (2 * n4 + 255) / 256));
    hipLaunchKernelGGL(fa_bwd_gqa_reduce_kernel, gr, dim3(256), 0, s, a.gqa_ws,
                       (short*)a.dk, (short*)a.dv, a.hkv, rep / G, a.skv, a.dh / 4, n4,
                       a.dk_s.b, a.dk_s.h, a.dk_s.s);
  }
}
#undef FA_BWD_ARGS
#undef FA_BWD_TAIL

}  // namespace pa
