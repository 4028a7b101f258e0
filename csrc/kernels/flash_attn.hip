// FlashAttention-2 forward + backward for gfx950 (CDNA4), bf16, head_dim
// 64/128, causal or full, MHA/GQA (GQA fwd; bwd requires hkv==h for the
// in-kernel path -- the Python layer repeats KV otherwise).
//
// MI355X-first design (NOT a port of the reference's dynloaded
// libflashattn -- paddle/phi/kernels/gpu/flash_attn_kernel.cu:41 is a
// dispatch shim; the math here is re-derived):
//   * MFMA 16x16x32 bf16 tiles; 8 waves/block; each wave owns 16 rows of
//     the 128-row Q (fwd, bwd-dq) / KV (bwd-dkv) block.
//   * fwd / bwd-dq: K / V^T staged in LDS with the XOR-16B swizzle (guide
//     §6 G4) so column-sliced ds_read_b128 is ~2-way conflict free, the
//     transposed tile written as a second copy.
//   * bwd-dkv: Q / dO staged once per tile by DMA into one image that is
//     read by rows (ds_read_b128) and by columns (ds_read_b64_tr_b16), two
//     buffers so the next tile loads under this tile's math (see the kernel).
//   * online softmax entirely in registers; row stats shared across the
//     16-lane C-tile groups via shfl_xor(1,2,4,8).
//   * LSE saved (fp32) for backward + ring/context-parallel merges.
//   * backward = 3 kernels (delta, dKV, dQ) -- no atomics, S recomputed
//     from Q,K,LSE per FA2.
#include "common.h"
#include "api.h"

namespace pa {

#define LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// lds byte offset helpers (row stride in bytes RS must be multiple of 32)
__device__ __forceinline__ unsigned lds_off(unsigned row, unsigned col_bytes,
                                            unsigned row_stride) {
  return row * row_stride + (col_bytes ^ ((row & 7u) << 4));
}

// read a 16B swizzled fragment (8 bf16) from LDS
__device__ __forceinline__ shortx8 lds_read8(const char* lds, unsigned row,
                                             unsigned col_elem, unsigned row_stride) {
  return *reinterpret_cast<const shortx8*>(lds + lds_off(row, col_elem * 2, row_stride));
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int D, bool CAUSAL>
__launch_bounds__(512)
__global__ void fa_fwd_kernel(const short* __restrict__ qg, const short* __restrict__ kg,
                              const short* __restrict__ vg, short* __restrict__ og,
                              float* __restrict__ lseg, int B, int H, int HKV,
                              int Sq, int Skv, float scale,
                              long long q_sb, long long q_sh, long long q_ss,
                              long long k_sb, long long k_sh, long long k_ss,
                              long long o_sb, long long o_sh, long long o_ss) {
  constexpr int NW = 8;         // waves per block (16 q rows each)
  constexpr int QB = 16 * NW, KB = 64;
  constexpr int NT = NW * 64;   // threads
  constexpr int NKK = D / 32;   // mfma k-steps over head dim
  constexpr int NDT = D / 16;   // output d tiles
  // LDS layout
  constexpr unsigned K_RS = D * 2;            // K tile row stride bytes
  constexpr unsigned VT_RS = KB * 2;          // V^T tile row stride
  __shared__ char k_lds[KB * D * 2];
  __shared__ char vt_lds[D * KB * 2];
  __shared__ char p_lds[NW * 16 * KB * 2];    // per-wave P tiles

  const int qblk = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int hkv = h / (H / HKV);
  const int q0 = qblk * QB;
  const long long qbase = (long long)b * q_sb + (long long)h * q_sh;
  const long long kbase = (long long)b * k_sb + (long long)hkv * k_sh;
  const long long obase = (long long)b * o_sb + (long long)h * o_sh;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wq = tid >> 6;          // wave id = which 16 q-rows
  const int l16 = lane & 15;        // col within C tile
  const int lg = lane >> 4;         // 16-lane group id (0..3)

  // Q fragments: A[i=row16][k] ; lane holds row l16, k = lg*8.. per kk-step
  shortx8 qf[NKK];
  {
    int row = q0 + wq * 16 + l16;
    bool ok = row < Sq;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      if (ok)
        qf[kk] = *reinterpret_cast<const shortx8*>(qg + qbase + (long long)row * q_ss + kk * 32 + lg * 8);
      else
        for (int i = 0; i < 8; ++i) qf[kk][i] = 0;
    }
  }

  floatx4 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = {0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -INFINITY; l_run[r] = 0.f; }

  const int kv_end = CAUSAL ? min(Skv, q0 + QB) : Skv;

  // K staging source offsets (pre-swizzled global address so the async
  // global_load_lds DMA lands the swizzled layout into linear LDS -- guide
  // §5 m173 pattern; the read side XORs the same mask back out)
  int k_row[KB * D / (NT * 8)], k_colp[KB * D / (NT * 8)];
#pragma unroll
  for (int it = 0; it < KB * D / (NT * 8); ++it) {
    int flat = it * NT * 8 + tid * 8;
    int row = flat / D, col = flat % D;
    k_row[it] = row;
    k_colp[it] = col ^ ((row & 7) << 3);
  }

  for (int kv0 = 0; kv0 < kv_end; kv0 += KB) {
    // ---- stage K tile [KB][D] (swizzled rows) -----------------------------
    if (kv0 + KB <= Skv) {
      // fast path: async DMA straight to LDS, no VGPR round-trip
#pragma unroll
      for (int it = 0; it < KB * D / (NT * 8); ++it) {
        const short* src = kg + kbase + (long long)(kv0 + k_row[it]) * k_ss + k_colp[it];
        char* dst = k_lds + it * NT * 16 + (tid >> 6) * 64 * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) unsigned int*)src,
                                         (__attribute__((address_space(3))) unsigned int*)dst,
                                         16, 0, 0);
      }
    } else {
      constexpr int elems = KB * D;
      for (int flat = tid * 8; flat < elems; flat += NT * 8) {
        int row = flat / D, col = flat % D;
        shortx8 val;
        if (kv0 + row < Skv)
          val = *reinterpret_cast<const shortx8*>(kg + kbase + (long long)(kv0 + row) * k_ss + col);
        else
          for (int i = 0; i < 8; ++i) val[i] = 0;
        *reinterpret_cast<shortx8*>(k_lds + lds_off(row, col * 2, K_RS)) = val;
      }
    }
    {
      constexpr int elems = KB * D;
      // ---- stage V^T tile [D][KB] ------------------------------------------
      for (int flat = tid * 8; flat < elems; flat += NT * 8) {
        int row = flat / D, col = flat % D;  // row=kv, col=d
        shortx8 val;
        if (kv0 + row < Skv)
          val = *reinterpret_cast<const shortx8*>(vg + kbase + (long long)(kv0 + row) * k_ss + col);
        else
          for (int i = 0; i < 8; ++i) val[i] = 0;
        // rotate write order by lane: without it all 16 lanes of a row-
        // group hit ONE bank (16-way conflict, the PMC hotspot); rotated
        // they spread over 8 banks (2-way).
        const int rot = threadIdx.x & 7;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int i = (j + rot) & 7;
          *reinterpret_cast<short*>(vt_lds + lds_off(col + i, row * 2, VT_RS)) = val[i];
        }
      }
    }
    __syncthreads();

    // ---- S = Q K^T --------------------------------------------------------
    floatx4 sacc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      sacc[nt] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        shortx8 kf = lds_read8(k_lds, nt * 16 + l16, kk * 32 + lg * 8, K_RS);
        sacc[nt] = mfma_bf16(qf[kk], kf, sacc[nt]);
      }
    }

    // ---- mask + scale + online softmax ------------------------------------
    const int q_abs = q0 + wq * 16 + lg * 4;  // + r
    const bool boundary = (kv0 + KB > Skv) || (CAUSAL && kv0 + KB > q_abs);
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (boundary) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int kv_abs = kv0 + nt * 16 + l16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float val = sacc[nt][r] * scale;
          if (kv_abs >= Skv || (CAUSAL && kv_abs > q_abs + r)) val = -INFINITY;
          sacc[nt][r] = val;
          mx[r] = fmaxf(mx[r], val);
        }
      }
    } else {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float val = sacc[nt][r] * scale;
          sacc[nt][r] = val;
          mx[r] = fmaxf(mx[r], val);
        }
    }
    float psum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mx[r] = group16_reduce(mx[r], MaxOp());
      // defer-max (guide T13): skip the O(NDT) rescale while the running
      // max hasn't grown by more than THR (P stays bounded by e^THR)
      const float THR = 8.f;
      if (mx[r] > m_run[r] + THR || m_run[r] == -INFINITY) {
        float m_new = fmaxf(m_run[r], mx[r]);
        float corr = (m_run[r] == -INFINITY) ? 0.f : __expf(m_run[r] - m_new);
        l_run[r] *= corr;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) oacc[dt][r] *= corr;
        m_run[r] = m_new;
      }
      psum[r] = 0.f;
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = (sacc[nt][r] == -INFINITY) ? 0.f : __expf(sacc[nt][r] - m_run[r]);
        sacc[nt][r] = p;
        psum[r] += p;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      psum[r] = group16_reduce(psum[r], SumOp());
      l_run[r] += psum[r];
    }

    // ---- P -> per-wave LDS (bf16, swizzled 128B rows) ---------------------
    char* pw = p_lds + wq * (16 * KB * 2);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        unsigned row = lg * 4 + r, col = nt * 16 + l16;
        *reinterpret_cast<short*>(pw + lds_off(row, col * 2, KB * 2)) = f2bf(sacc[nt][r]);
      }
    }
    LGKM0();

    // ---- O += P V ---------------------------------------------------------
#pragma unroll
    for (int kk = 0; kk < KB / 32; ++kk) {
      shortx8 pf = lds_read8(pw, l16, kk * 32 + lg * 8, KB * 2);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        shortx8 vf = lds_read8(vt_lds, dt * 16 + l16, kk * 32 + lg * 8, VT_RS);
        oacc[dt] = mfma_bf16(pf, vf, oacc[dt]);
      }
    }
    __syncthreads();
  }

  // ---- finalize: O /= l ; write O + LSE -----------------------------------
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int row = q0 + wq * 16 + lg * 4 + r;
    if (row >= Sq) continue;
    float inv_l = (l_run[r] > 0.f) ? 1.f / l_run[r] : 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      og[obase + (long long)row * o_ss + dt * 16 + l16] = f2bf(oacc[dt][r] * inv_l);
    if (l16 == 0)
      lseg[(long long)(b * H + h) * Sq + row] =
          (l_run[r] > 0.f) ? m_run[r] + __logf(l_run[r]) : -INFINITY;
  }
}

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

static void fa_bwd_delta(const void* dout, const void* o, float* delta,
                         int64_t bh_h, int64_t sq, long long rows, int64_t dh,
                         long long do_sb, long long do_sh, long long do_ss,
                         long long o_sb, long long o_sh, long long o_ss,
                         hipStream_t s) {
  const int rows_per_iter = (256 / (int)(dh / 8)) * 4;
  dim3 dgrid((unsigned)hmin<long long>(2048LL, (rows + rows_per_iter - 1) / rows_per_iter));
  if (dh == 128)
    hipLaunchKernelGGL((fa_bwd_delta_kernel<128>), dgrid, dim3(256), 0, s,
                       (const short*)dout, (const short*)o, delta, (int)bh_h,
                       (int)sq, rows, do_sb, do_sh, do_ss, o_sb, o_sh, o_ss);
  else
    hipLaunchKernelGGL((fa_bwd_delta_kernel<64>), dgrid, dim3(256), 0, s,
                       (const short*)dout, (const short*)o, delta, (int)bh_h,
                       (int)sq, rows, do_sb, do_sh, do_ss, o_sb, o_sh, o_ss);
}

// delta alone (tests / benchmarks); strides as in flash_attn_bwd
void flash_attn_bwd_delta(const void* dout, const void* o, float* delta,
                          int64_t b, int64_t h, int64_t sq, int64_t dh,
                          const int64_t* dos, const int64_t* os, hipStream_t s) {
  fa_bwd_delta(dout, o, delta, h, sq, b * h * sq, dh, dos[0], dos[1], dos[2],
               os[0], os[1], os[2], s);
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

template <int D, bool CAUSAL>
__launch_bounds__(512)
__global__ void fa_bwd_dkv_kernel(const short* __restrict__ dog, const short* __restrict__ qg,
                                  const short* __restrict__ kg, const short* __restrict__ vg,
                                  const float* __restrict__ lseg, const float* __restrict__ deltag,
                                  short* __restrict__ dkg, short* __restrict__ dvg,
                                  int B, int H, int Sq, int Skv, float scale,
                                  long long q_sb, long long q_sh, long long q_ss,
                                  long long k_sb, long long k_sh, long long k_ss,
                                  long long do_sb, long long do_sh, long long do_ss,
                                  long long dk_sb, long long dk_sh, long long dk_ss) {
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
  const int b = bh / H, h = bh % H;
  const long long qbase = (long long)b * q_sb + (long long)h * q_sh;
  const long long dobase = (long long)b * do_sb + (long long)h * do_sh;
  const long long kvbase = (long long)b * k_sb + (long long)h * k_sh;
  const long long dkbase = (long long)b * dk_sb + (long long)h * dk_sh;
  const long long lse_base = ((long long)bh) * Sq;

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
  for (int q0 = q_start; q0 < Sq; q0 += QB) {
    // Tile q0 was issued one tile ago (or in the prologue) and nothing newer
    // is in flight, so the counted wait is vmcnt(0).  The one barrier per
    // tile then says both "tile q0 has landed for every wave" and "every
    // wave is done reading tile q0-QB", which frees the other buffer.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned boff = cur * (2 * TILE);
    const char* q_t = lds + boff;
    float lse_v[4], delta_v[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) { lse_v[nt] = lse_n[nt]; delta_v[nt] = delta_n[nt]; }
    if (q0 + QB < Sq) {
      stage(q0 + QB, lds + (cur ^ 1) * (2 * TILE));
      load_stats(q0 + QB, lse_n, delta_n);
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
// backward dQ: block owns a 64-row Q tile; iterate kv tiles.
// ---------------------------------------------------------------------------
template <int D, bool CAUSAL>
__launch_bounds__(512)
__global__ void fa_bwd_dq_kernel(const short* __restrict__ dog, const short* __restrict__ qg,
                                 const short* __restrict__ kg, const short* __restrict__ vg,
                                 const float* __restrict__ lseg, const float* __restrict__ deltag,
                                 short* __restrict__ dqg, int B, int H, int Sq, int Skv,
                                 float scale,
                                 long long q_sb, long long q_sh, long long q_ss,
                                 long long k_sb, long long k_sh, long long k_ss,
                                 long long do_sb, long long do_sh, long long do_ss,
                                 long long dq_sb, long long dq_sh, long long dq_ss) {
  constexpr int NW = 8;               // waves; block owns NW*16 q rows
  constexpr int NT = NW * 64;
  constexpr int QEXT = NW * 16;
  constexpr int KB = 64;
  constexpr int NKK = D / 32;
  constexpr int NDT = D / 16;
  constexpr unsigned NAT_RS = D * 2;
  constexpr unsigned TR_RS = KB * 2;
  __shared__ char k_lds[KB * D * 2];
  __shared__ char v_lds[KB * D * 2];
  __shared__ char kt_lds[D * KB * 2];
  __shared__ char ps_lds[NW * 16 * KB * 2];

  const int qblk = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int q0 = qblk * QEXT;
  const long long qbase = (long long)b * q_sb + (long long)h * q_sh;
  const long long dobase = (long long)b * do_sb + (long long)h * do_sh;
  const long long dqbase = (long long)b * dq_sb + (long long)h * dq_sh;
  const long long kvbase = (long long)b * k_sb + (long long)h * k_sh;
  const long long lse_base = ((long long)bh) * Sq;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wq = tid >> 6;
  const int l16 = lane & 15;
  const int lg = lane >> 4;

  shortx8 qf[NKK], dof[NKK];
  {
    int row = q0 + wq * 16 + l16;
    bool ok = row < Sq;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      if (ok) {
        qf[kk] = *reinterpret_cast<const shortx8*>(qg + qbase + (long long)row * q_ss + kk * 32 + lg * 8);
        dof[kk] = *reinterpret_cast<const shortx8*>(dog + dobase + (long long)row * do_ss + kk * 32 + lg * 8);
      } else {
        for (int i = 0; i < 8; ++i) { qf[kk][i] = 0; dof[kk][i] = 0; }
      }
    }
  }
  float lse_r[4], delta_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int row = q0 + wq * 16 + lg * 4 + r;
    lse_r[r] = (row < Sq) ? lseg[lse_base + row] : INFINITY;
    delta_r[r] = (row < Sq) ? deltag[lse_base + row] : 0.f;
  }

  floatx4 dq_acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) dq_acc[dt] = {0.f, 0.f, 0.f, 0.f};

  const int kv_end = CAUSAL ? min(Skv, q0 + QEXT) : Skv;
  int n_row[KB * D / (NT * 8)], n_colp[KB * D / (NT * 8)];
#pragma unroll
  for (int it = 0; it < KB * D / (NT * 8); ++it) {
    int flat = it * NT * 8 + tid * 8;
    int row = flat / D, col = flat % D;
    n_row[it] = row;
    n_colp[it] = col ^ ((row & 7) << 3);
  }
  for (int kv0 = 0; kv0 < kv_end; kv0 += KB) {
    if (kv0 + KB <= Skv) {
#pragma unroll
      for (int it = 0; it < KB * D / (NT * 8); ++it) {
        const short* ksrc = kg + kvbase + (long long)(kv0 + n_row[it]) * k_ss + n_colp[it];
        const short* vsrc = vg + kvbase + (long long)(kv0 + n_row[it]) * k_ss + n_colp[it];
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)ksrc,
            (__attribute__((address_space(3))) unsigned int*)(k_lds + it * NT * 16 + (tid >> 6) * 64 * 16),
            16, 0, 0);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)vsrc,
            (__attribute__((address_space(3))) unsigned int*)(v_lds + it * NT * 16 + (tid >> 6) * 64 * 16),
            16, 0, 0);
      }
      constexpr int elems = KB * D;
      const int rot = threadIdx.x & 7;
      for (int flat = tid * 8; flat < elems; flat += NT * 8) {
        int row = flat / D, col = flat % D;
        shortx8 kv_ = *reinterpret_cast<const shortx8*>(kg + kvbase + (long long)(kv0 + row) * k_ss + col);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int i = (j + rot) & 7;
          *reinterpret_cast<short*>(kt_lds + lds_off(col + i, row * 2, TR_RS)) = kv_[i];
        }
      }
    } else {
      constexpr int elems = KB * D;
      for (int flat = tid * 8; flat < elems; flat += NT * 8) {
        int row = flat / D, col = flat % D;
        shortx8 kv_, vv;
        if (kv0 + row < Skv) {
          kv_ = *reinterpret_cast<const shortx8*>(kg + kvbase + (long long)(kv0 + row) * k_ss + col);
          vv = *reinterpret_cast<const shortx8*>(vg + kvbase + (long long)(kv0 + row) * k_ss + col);
        } else {
          for (int i = 0; i < 8; ++i) { kv_[i] = 0; vv[i] = 0; }
        }
        *reinterpret_cast<shortx8*>(k_lds + lds_off(row, col * 2, NAT_RS)) = kv_;
        *reinterpret_cast<shortx8*>(v_lds + lds_off(row, col * 2, NAT_RS)) = vv;
        const int rot = threadIdx.x & 7;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int i = (j + rot) & 7;
          *reinterpret_cast<short*>(kt_lds + lds_off(col + i, row * 2, TR_RS)) = kv_[i];
        }
      }
    }
    __syncthreads();

    const int q_abs0 = q0 + wq * 16 + lg * 4;
    floatx4 ds[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      floatx4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        shortx8 kfr = lds_read8(k_lds, nt * 16 + l16, kk * 32 + lg * 8, NAT_RS);
        s = mfma_bf16(qf[kk], kfr, s);
        shortx8 vfr = lds_read8(v_lds, nt * 16 + l16, kk * 32 + lg * 8, NAT_RS);
        dp = mfma_bf16(dof[kk], vfr, dp);
      }
      const int kv_abs = kv0 + nt * 16 + l16;
      const bool bnd = (kv0 + KB > Skv) || (CAUSAL && kv0 + KB > q_abs0);
      if (bnd) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = __expf(s[r] * scale - lse_r[r]);
          if (kv_abs >= Skv || (CAUSAL && kv_abs > q_abs0 + r)) p = 0.f;
          ds[nt][r] = p * (dp[r] - delta_r[r]) * scale;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = __expf(s[r] * scale - lse_r[r]);
          ds[nt][r] = p * (dp[r] - delta_r[r]) * scale;
        }
      }
    }

    char* pw = ps_lds + wq * (16 * KB * 2);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<short*>(pw + lds_off(lg * 4 + r, (nt * 16 + l16) * 2, KB * 2)) =
            f2bf(ds[nt][r]);
    LGKM0();

#pragma unroll
    for (int kk = 0; kk < KB / 32; ++kk) {
      shortx8 pa = lds_read8(pw, l16, kk * 32 + lg * 8, KB * 2);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        shortx8 bfr = lds_read8(kt_lds, dt * 16 + l16, kk * 32 + lg * 8, TR_RS);
        dq_acc[dt] = mfma_bf16(pa, bfr, dq_acc[dt]);
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int row = q0 + wq * 16 + lg * 4 + r;
    if (row >= Sq) continue;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      dqg[dqbase + (long long)row * dq_ss + dt * 16 + l16] = f2bf(dq_acc[dt][r]);
  }
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
void flash_attn_fwd(const void* q, const void* k, const void* v, void* o,
                    float* lse, int64_t b, int64_t h, int64_t hkv, int64_t sq,
                    int64_t skv, int64_t dh, float scale, bool causal,
                    const int64_t* qs, const int64_t* ks, const int64_t* os,
                    hipStream_t s) {
  dim3 grid((unsigned)cdiv((int)sq, 128), (unsigned)(b * h));
  dim3 blk(512);
#define FAF(D, C)                                                             \
  hipLaunchKernelGGL((fa_fwd_kernel<D, C>), grid, blk, 0, s, (const short*)q, \
                     (const short*)k, (const short*)v, (short*)o, lse,        \
                     (int)b, (int)h, (int)hkv, (int)sq, (int)skv, scale,      \
                     qs[0], qs[1], qs[2], ks[0], ks[1], ks[2],                \
                     os[0], os[1], os[2])
  if (dh == 128) { if (causal) FAF(128, true); else FAF(128, false); }
  else           { if (causal) FAF(64, true);  else FAF(64, false); }
#undef FAF
}

void flash_attn_bwd(const void* dout, const void* q, const void* k,
                    const void* v, const void* o, const float* lse,
                    void* dq, void* dk, void* dv, float* delta, int64_t b,
                    int64_t h, int64_t hkv, int64_t sq, int64_t skv,
                    int64_t dh, float scale, bool causal,
                    const int64_t* qs, const int64_t* ks, const int64_t* dos,
                    const int64_t* os, const int64_t* dqs, const int64_t* dks,
                    const void* mask, const int64_t* ms, float pdrop,
                    uint64_t seed, uint64_t offset, hipStream_t s) {
  fa_bwd_delta(dout, o, delta, h, sq, b * h * sq, dh, dos[0], dos[1], dos[2],
               os[0], os[1], os[2], s);

  dim3 gkv((unsigned)(b * h), (unsigned)cdiv((int)skv, 128));
  dim3 gq((unsigned)cdiv((int)sq, 128), (unsigned)(b * h));
  // The 16x16 dKV kernel is the default: both 32x32 rewrites measured
  // slower (combined/transposed-output: 146 TF bwd at occupancy 1;
  // occupancy-2 split with global A-frags: 95 TF; 16x16 baseline: 168 TF).
  // PA_FA_DKV32=1 opts into the 32x32 path for future experiments.
  static const bool dkv16_env = [] {
    const char* e = getenv("PA_FA_DKV32");
    return !(e && e[0] == '1');
  }();
  // the 16x16 dKV kernel has no mask/dropout path; route those to dkv32
  const bool use_dkv16 = dkv16_env && mask == nullptr && pdrop <= 0.f;
#define FAB(D, C)                                                              \
  do {                                                                         \
    if (use_dkv16)                                                             \
      hipLaunchKernelGGL((fa_bwd_dkv_kernel<D, C>), gkv, dim3(512), 0, s,      \
                         (const short*)dout, (const short*)q, (const short*)k, \
                         (const short*)v, lse, delta, (short*)dk, (short*)dv,  \
                         (int)b, (int)h, (int)sq, (int)skv, scale,             \
                         qs[0], qs[1], qs[2], ks[0], ks[1], ks[2],             \
                         dos[0], dos[1], dos[2], dks[0], dks[1], dks[2]);      \
    else                                                                       \
      flash_attn_bwd_dkv32(dout, q, k, v, lse, delta, dk, dv, b, h, sq, skv,   \
                           dh, scale, causal, qs, ks, dos, dks, mask, ms,      \
                           pdrop, seed, offset, s);                            \
    flash_attn_bwd_dq32(dout, q, k, v, lse, delta, dq, b, h, sq, skv, dh,     \
                        scale, causal, qs, ks, dos, dqs, mask, ms, pdrop,      \
                        seed, offset, s);                                      \
  } while (0)
  if (dh == 128) { if (causal) FAB(128, true); else FAB(128, false); }
  else           { if (causal) FAB(64, true);  else FAB(64, false); }
#undef FAB
}

void flash_attn_varlen_bwd(const void* dout, const void* q, const void* k,
                           const void* v, const void* o, const float* lse,
                           void* dq, void* dk, void* dv, float* delta,
                           int64_t h, int64_t total_q, int64_t total_k,
                           int64_t dh, float scale, bool causal,
                           int64_t nqblocks, int64_t nkvblocks,
                           const int* cu_q, const int* cu_k, const int* qbmap,
                           const int* kvbmap, float pdrop, uint64_t seed,
                           uint64_t offset, hipStream_t s) {
  // delta[h, total_q] = rowsum(do * o) over the packed [total, H, D] layout
  const long long ss = h * dh;
  fa_bwd_delta(dout, o, delta, h, total_q, h * total_q, dh, 0, dh, ss, 0, dh,
               ss, s);
  flash_attn_varlen_bwd32(dout, q, k, v, lse, delta, dq, dk, dv, h, total_q,
                          total_k, dh, scale, causal, nqblocks, nkvblocks,
                          cu_q, cu_k, qbmap, kvbmap, pdrop, seed, offset, s);
}

}  // namespace pa
