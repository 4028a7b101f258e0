// Shared by the flash-attention kernels (fa_fwd32.hip, fa_bwd.hip): the
// 32x32-MFMA fragment helpers, the per-block geometry of the forward kernel
// and the runtime -> compile-time dispatch of the launchers.  The forward
// kernel takes pa::FaArgs (api.h) by value as its one argument; the backward
// kernels keep scalar arguments (docs/KERNELS.md, launch path), the GQA ones
// of hkv != h last.
#pragma once
#include <type_traits>

#include "common.h"
#include "api.h"

namespace pa {

typedef __attribute__((ext_vector_type(16))) float floatx16;
typedef __attribute__((ext_vector_type(2))) int intx2;

// C/D layout of the 32x32 tile (measured): col = lane&31,
// row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
__device__ __forceinline__ floatx16 mfma32_bf16(shortx8 a, shortx8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ unsigned lds_off32(unsigned row, unsigned col_bytes,
                                              unsigned row_stride) {
  return row * row_stride + (col_bytes ^ ((row & 7u) << 4));
}

// ---------------------------------------------------------------------------
// K / V image of fa_fwd32_kernel and fa_bwd_dq32_kernel: the natural [64][D]
// tile, landed once by DMA, with the 16-byte chunk index of each row XORed by
// fa_kv_swz(row).  It is read by rows (ds_read_b128, A operand of S^T / dP^T,
// k = d) and by columns (ds_read_b64_tr_b16, B operand of P V / dS K, k = kv).
//
// Bank rule: a 256-byte bank row; ds_read_b64_tr_b16 conflicts inside a
// 32-lane half, ds_read_b128 inside its 16-lane groups {0-3,12-15,20-27},
// {4-11,16-19,28-31} (+32).
//   transposed read of the 32x32x16 B operand: a half takes rows r0+{0..3}
//     (r0 a multiple of 4), 64 bytes per row, chunks 4*dt..4*dt+3 -> the 4
//     rows must land on 4 different 64-byte quarters of the bank row;
//   row read of the 32x32x16 A operand: a group takes rows {0-3,12-15,20-27}
//     or {4-11,16-19,28-31} at one chunk -> 16 different 16-byte slots.
// D = 128: the quarter comes from row&3, the slot inside it from (row>>3)&3;
// the four 4-row runs of either group have four different row>>3.  Rows r
// and r+4 of an aligned 8-row group, and rows 32 apart, keep the XOR, so the
// second half of a B fragment and the k-step after next are immediate
// offsets; rows 16 apart do not, so a d tile has one address register for
// even and one for odd k-steps.  (The guide's image (b), slot bits
// (row>>2)&3, is as conflict-free but needs another register for rows +4.)
// D = 64 has two rows per bank row: row&1 picks the half, (row>>1)&1 the
// quarter inside it, (row>>3)&3 the slot; the same properties hold.
// ---------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ unsigned fa_kv_swz(unsigned row) {
  if constexpr (D == 128)
    return ((row & 3u) << 2) | ((row >> 3) & 3u);
  else
    return (((row >> 1) & 1u) << 2) | ((row >> 3) & 3u);
}

// byte offset of 16-byte chunk `ch` of row `row`; the DMA source column, the
// tail tile's stores and both kinds of read go through it
template <int D>
__device__ __forceinline__ unsigned fa_kv_off(unsigned row, unsigned ch) {
  return row * (D * 2) + ((ch ^ fa_kv_swz<D>(row)) << 4);
}

// Stage the [64][D] K tile at kv0 into buf and the V tile into buf + 64*D*2,
// by a block of NT threads.  A whole tile goes by DMA (global_load_lds 16 B;
// the target is lane-linear, so the XOR sits on the source column: the lane
// that fills chunk position c of row r fetches chunk c ^ swz(r)).  The tail
// tile takes guarded 16-byte loads with zero fill and ordinary stores, so no
// address past the tensor's last row is formed into a load.
template <int D, int NT>
__device__ __forceinline__ void fa_stage_kv(char* buf, const short* __restrict__ kg,
                                            const short* __restrict__ vg, long long base,
                                            long long k_ss, int kv0, int Skv_e, int tid) {
  constexpr int KB = 64;
  constexpr int TILE = KB * D * 2;
  if (kv0 + KB <= Skv_e) {
#pragma unroll
    for (int it = 0; it < KB * D / (NT * 8); ++it) {
      const int flat = it * NT * 8 + tid * 8;
      const int row = flat / D, col = flat % D;
      const long long src = base + (long long)(kv0 + row) * k_ss
                          + (col ^ (int)(fa_kv_swz<D>(row) << 3));
      char* dst = buf + it * NT * 16 + (tid >> 6) * 64 * 16;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(kg + src),
          (__attribute__((address_space(3))) unsigned int*)dst, 16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(vg + src),
          (__attribute__((address_space(3))) unsigned int*)(dst + TILE), 16, 0, 0);
    }
  } else {
    for (int flat = tid * 8; flat < KB * D; flat += NT * 8) {
      const int row = flat / D, col = flat % D;
      shortx8 kv_, vv;
      if (kv0 + row < Skv_e) {
        kv_ = *reinterpret_cast<const shortx8*>(kg + base + (long long)(kv0 + row) * k_ss + col);
        vv = *reinterpret_cast<const shortx8*>(vg + base + (long long)(kv0 + row) * k_ss + col);
      } else {
        for (int i = 0; i < 8; ++i) { kv_[i] = 0; vv[i] = 0; }
      }
      const unsigned o = fa_kv_off<D>(row, col >> 3);
      *reinterpret_cast<shortx8*>(buf + o) = kv_;
      *reinterpret_cast<shortx8*>(buf + TILE + o) = vv;
    }
  }
}

// LDS address of the lane for the transposed reads of the 32x32x16 B operand
// B[k = r0 + 8*hi + 0..3][n = 32*dt + l32] of an image at LDS address `img`,
// r0 = 0 or 16, less the r0 rows (the reads add them back as an immediate):
// ds_read_b64_tr_b16 works per 16-lane group; lane 4q+p passes the address of
// row q, columns 4p..4p+3 of a 4-row x 16-column block, lane i gets column i
// with row j in element j.  Group g holds hi = g>>1 and columns 16*(g&1)+..
template <int D>
__device__ __forceinline__ unsigned fa_tr_addr(unsigned img, int lane, int dt, int r0) {
  const unsigned g = lane >> 4, q = (lane >> 2) & 3u, p = lane & 3u;
  return img + fa_kv_off<D>(r0 + 8 * (g >> 1) + q, 4 * dt + 2 * (g & 1u) + (p >> 1))
       + ((p & 1u) << 3) - r0 * (D * 2);
}

// B fragments B[k = 16*ks + 8*hi + 0..7][n = 32*dt + l32] of all D/32 d tiles
// in one statement: a[dt] from fa_tr_addr with r0 = 16*(ks&1) (plus the
// buffer's offset), LO the byte offset of the image and of row 16*ks in it,
// rows +4..7 are 4 rows on.
// EXEC must be all ones.  Inline asm that ends in its own lgkmcnt(0): as a
// builtin each read is waited for on its own and the first one of a tile
// draws a vmcnt(0) that drains the prefetch of the next tile.
template <int D, int LO>
__device__ __forceinline__ void fa_tr_read(shortx8 (&b)[D / 32], const unsigned (&a)[D / 32]) {
  constexpr int HI = LO + 4 * D * 2;
  static_assert(HI < 65536, "ds offset field");
  if constexpr (D == 128) {
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
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "n"(LO), "n"(HI)
        : "memory");
    b[0] = __builtin_shufflevector(l0, h0, 0, 1, 2, 3, 4, 5, 6, 7);
    b[1] = __builtin_shufflevector(l1, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    b[2] = __builtin_shufflevector(l2, h2, 0, 1, 2, 3, 4, 5, 6, 7);
    b[3] = __builtin_shufflevector(l3, h3, 0, 1, 2, 3, 4, 5, 6, 7);
  } else {
    shortx4 l0, h0, l1, h1;
    asm volatile(
        "ds_read_b64_tr_b16 %0, %4 offset:%6\n\t"
        "ds_read_b64_tr_b16 %1, %4 offset:%7\n\t"
        "ds_read_b64_tr_b16 %2, %5 offset:%6\n\t"
        "ds_read_b64_tr_b16 %3, %5 offset:%7\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(l0), "=&v"(h0), "=&v"(l1), "=&v"(h1)
        : "v"(a[0]), "v"(a[1]), "n"(LO), "n"(HI)
        : "memory");
    b[0] = __builtin_shufflevector(l0, h0, 0, 1, 2, 3, 4, 5, 6, 7);
    b[1] = __builtin_shufflevector(l1, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  }
}

__device__ __forceinline__ int pack_bf2(float a, float b) {
  unsigned lo = (unsigned short)f2bf(a);
  unsigned hi = (unsigned short)f2bf(b);
  return (int)(lo | (hi << 16));
}

// What a block of a 32x32 kernel works on.  grid.x = batch * head, grid.y =
// 128-row block.  Dense: the
// whole [sq, skv] problem of (b, h), r0 chosen by the kernel.  Varlen: b = 0,
// the block map names the sequence and r0, the row of the block inside it;
// q_tok0 / k_tok0 are the sequence's first packed tokens, Sq_e / Skv_e its
// lengths, and causal is bottom-right aligned by cdelta = Skv_e - Sq_e.
struct FaBlock {
  int b, h, r0, Sq_e, Skv_e, cdelta, q_tok0, k_tok0;
};

template <bool VARLEN>
__device__ __forceinline__ FaBlock fa_block(const FaArgs& a, const int* bmap,
                                            int dense_r0) {
  FaBlock g;
  const int bh = blockIdx.x, blk = blockIdx.y;
  if (VARLEN) {
    const int seq = bmap[2 * blk];
    g.b = 0; g.h = bh;
    g.r0 = bmap[2 * blk + 1];
    g.q_tok0 = a.cu_q[seq];
    g.k_tok0 = a.cu_k[seq];
    g.Sq_e = a.cu_q[seq + 1] - g.q_tok0;
    g.Skv_e = a.cu_k[seq + 1] - g.k_tok0;
    g.cdelta = g.Skv_e - g.Sq_e;
  } else {
    g.b = bh / a.h; g.h = bh % a.h;
    g.r0 = dense_r0;
    g.q_tok0 = 0; g.k_tok0 = 0;
    g.Sq_e = a.sq; g.Skv_e = a.skv;
    g.cdelta = 0;
  }
  return g;
}

// element offset of row 0 of the block's (batch | sequence, head)
__device__ __forceinline__ long long fa_base(const FaBlock& g, const FaStride& s,
                                             int head, int tok0) {
  return (long long)g.b * s.b + (long long)head * s.h + (long long)tok0 * s.s;
}

// runtime (dh, causal, masked, dropped) -> f(D, CAUSAL, MASKED, DROPOUT) with
// std::integral_constant arguments
template <class F>
inline void fa_bool(bool v, F&& f) {
  if (v) f(std::true_type{}); else f(std::false_type{});
}

template <class F>
inline void fa_dispatch(const FaArgs& a, F&& f) {
  fa_bool(a.dh == 128, [&](auto d128) {
    fa_bool(a.causal, [&](auto c) {
      fa_bool(a.mask != nullptr, [&](auto m) {
        fa_bool(a.pdrop > 0.f, [&](auto p) {
          f(std::integral_constant<int, decltype(d128)::value ? 128 : 64>{}, c, m, p);
        });
      });
    });
  });
}

// the backward's dispatch: fa_dispatch plus GQA = (hkv != h)
template <class F>
inline void fa_dispatch_gqa(const FaArgs& a, F&& f) {
  fa_bool(a.hkv != a.h, [&](auto g) {
    fa_dispatch(a, [&](auto D, auto C, auto M, auto P) { f(D, C, M, P, g); });
  });
}

}  // namespace pa
