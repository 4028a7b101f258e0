// Shared by the flash-attention kernels (fa_fwd32.hip, fa_bwd.hip): the
// 32x32-MFMA fragment helpers, the per-block geometry of the forward kernel
// and the runtime -> compile-time dispatch of the launchers.  The forward
// kernel takes pa::FaArgs (api.h) by value as its one argument; the backward
// kernels keep scalar arguments (docs/KERNELS.md, launch path).
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

// 16-granule variant for 256 B rows (D=128 tiles): fragment reads pull 32
// DIFFERENT rows at one column, so an 8-way spread leaves 4-way bank
// conflicts (measured ~1 conflict-cycle/busy-cycle); 16 granules reach the
// b128 2-way floor.
__device__ __forceinline__ unsigned lds_off32w(unsigned row, unsigned col_bytes,
                                               unsigned row_stride, unsigned mask) {
  return row * row_stride + (col_bytes ^ ((row & mask) << 4));
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

}  // namespace pa
