// Paged prefill attention for gfx950: q_len >= 1 new tokens per sequence
// attend to the paged KV cache (bf16 or int8 codes), bottom-right causal
// (docs/KERNELS.md "paged prefill attention").  The kernel behind chunked
// prefill, prefix reuse and speculative-decode verification; at q_len = 1 it
// is an MFMA GQA decode tile.
//
// Row space: for one (sequence b, kv head) the query rows are r = i * G + g
// (token i, head g of the group, G = H / HKV); all of them share one K/V
// stream.  A 256-thread block owns 64 consecutive rows, 16 per wave; grid =
// (ceil(max_q * G / 64), HKV, B).  Blocks past q_len_b * G leave before any
// load; surplus rows inside a live block compute on zero q and store nothing.
//
// Per step the block stages 64 cached positions as bf16 into two LDS images
// (int8 codes are converted while staging: |code| <= 127 is exact in bf16);
// the global loads of step t+1 are issued before the math of step t.
//   S^T = mfma_16x16x32(K, Q): a lane holds one query column (lane & 15) and
//     positions 16*tt + 4*(lane >> 4) + r in register r of sub-tile tt, so
//     row max / sum are per-lane reductions plus xor-shuffles over 16 and 32.
//   O^T += mfma_16x16x32(V^T, P^T): P^T is the B operand straight from the
//     score registers; the k order of a step is the accumulator's row order,
//     k = 8*(lane >> 4) + j  <->  position 32*u + 16*(j >> 2) + 4*(lane >> 4)
//     + (j & 3), and V^T comes in the same order from two ds_read_b64_tr_b16
//     blocks (rows 32u + 4*(lane >> 4) + 0..3 and 16 rows further on).
// Scales act on the result: s = (sum q * code) * (d_k[pos] * scale),
// P~ = bf16(p * d_v[pos]), l sums the fp32 p.  Finite -1e30 sentinel.
#include <type_traits>

#include "common.h"
#include "api.h"

namespace pa {
namespace {

// Both images are natural [64][D] bf16 tiles whose 16-byte chunk index is
// XORed per row.  Bank rule: docs/KERNELS.md "dK/dV backward -> Image".
//   K, row reads of the 16x16x32 A operand: a ds_read_b128 group takes rows
//     {0-3, 12-15} at chunk c and rows {4-11} at chunk c ^ 1; XOR with the
//     row (D = 128) or with row >> 1 beside the row & 1 half of the 256-byte
//     bank row (D = 64) lands the 16 lanes on 16 different slots.
//   V, transposed reads: a 32-lane half takes 8 consecutive rows 8m .. 8m+7
//     at one chunk pair (2n, 2n+1); pair bits from row & 7 (D = 128) or from
//     (row >> 1) & 3 beside the row & 1 half (D = 64) give 8 different
//     32-byte pairs.  The XOR is the same for rows 16 apart, so the reads of
//     a d tile differ by immediates only.
template <int D>
__device__ __forceinline__ unsigned pf_off_k(unsigned row, unsigned ch) {
  const unsigned x = D == 128 ? (row & 15u) : ((row >> 1) & 7u);
  return row * (D * 2) + ((ch ^ x) << 4);
}
template <int D>
__device__ __forceinline__ unsigned pf_off_v(unsigned row, unsigned ch) {
  const unsigned x = D == 128 ? ((row & 7u) << 1) : (((row >> 1) & 3u) << 1);
  return row * (D * 2) + ((ch ^ x) << 4);
}

// ds_read_b64_tr_b16: per 16-lane group, lane 4q+p passes the address of row
// q, columns 4p..4p+3 of a 4-row x 16-column block; lane i gets column i, row
// j in element j.  EXEC must be all ones.  One statement reads the A
// fragments of four d tiles for one k-step: a0..a3 address the lane's row and
// 8 bytes in the block at rows 4*(lane >> 4) + 0..3 of d tiles n..n+3, LO /
// HI are the byte offsets of the step's two row blocks.
template <int LO, int HI>
__device__ __forceinline__ void pf_tr_read4(shortx8 (&v)[4], unsigned a0,
                                            unsigned a1, unsigned a2,
                                            unsigned a3) {
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
      : "=&v"(l0), "=&v"(h0), "=&v"(l1), "=&v"(h1), "=&v"(l2), "=&v"(h2),
        "=&v"(l3), "=&v"(h3)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "n"(LO), "n"(HI)
      : "memory");
  v[0] = __builtin_shufflevector(l0, h0, 0, 1, 2, 3, 4, 5, 6, 7);
  v[1] = __builtin_shufflevector(l1, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  v[2] = __builtin_shufflevector(l2, h2, 0, 1, 2, 3, 4, 5, 6, 7);
  v[3] = __builtin_shufflevector(l3, h3, 0, 1, 2, 3, 4, 5, 6, 7);
}

// two int8 codes (bytes i, i+1 of w) as a pair of bf16: exact
__device__ __forceinline__ unsigned pf_codes2bf(unsigned w, int i) {
  const float lo = (float)(int)(signed char)(w >> (8 * i));
  const float hi = (float)(int)(signed char)(w >> (8 * i + 8));
  return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
}

template <int D, bool INT8>
__launch_bounds__(256)
__global__ void paged_prefill_kernel(const PrefillAttnArgs a) {
  constexpr int TP = 64;                     // positions per step
  constexpr int RS = D * 2;                  // bytes of an image row
  constexpr int IMG = TP * RS;               // bytes of an image
  constexpr int CW = INT8 ? 16 : 8;          // elements of a 16-byte load
  constexpr int NCH = D / CW;                // loads per cached row
  constexpr int NIT = TP * NCH / 256;        // loads per thread and image
  constexpr int NKS = D / 32, NDT = D / 16;
  static_assert(TP * NCH % 256 == 0, "whole loads per thread");
  using cache_t = std::conditional_t<INT8, signed char, short>;
  // one array: K image, V image, d_k * scale and d_v per position, the mask
  // of positions that hold data
  __shared__ __attribute__((aligned(16))) char lds[2 * IMG + 2 * TP * 4 + 16];
  char* const kimg = lds;
  char* const vimg = lds + IMG;
  float* const kmul = reinterpret_cast<float*>(lds + 2 * IMG);
  float* const vmul = kmul + TP;
  unsigned long long* const okmask =
      reinterpret_cast<unsigned long long*>(lds + 2 * IMG + 2 * TP * 4);

  const cache_t* __restrict__ kcache = (const cache_t*)a.kcache;
  const cache_t* __restrict__ vcache = (const cache_t*)a.vcache;
  const int H = a.h, HKV = a.hkv, bs = a.bs, max_blocks = a.max_blocks;
  const int G = H / HKV;
  const int b = blockIdx.z, hkv = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, hq = lane >> 4;

  const int q0 = a.cu_q[b];
  const int q_len = a.cu_q[b + 1] - q0;
  const long long rows = (long long)q_len * G;
  const long long r0 = (long long)blockIdx.x * 64;
  if (q_len <= 0 || r0 >= rows) return;      // before any load
  // never walk past the table
  const int S = max(0, min(a.seq_lens[b], max_blocks * bs));
  const long long base = (long long)S - q_len;  // position of token 0

  // last visible position of the block's / the wave's last live row, and of
  // the wave's first row; -1: nothing to do
  auto row_lim = [&](long long r) -> int {
    return (int)max(-1LL, base + r / G);
  };
  const int maxlim = row_lim(min(rows - 1, r0 + 63));
  const long long rw0 = r0 + 16 * wid;
  const int wmaxlim = rw0 < rows ? row_lim(min(rows - 1, rw0 + 15)) : -1;
  const int wminlim = rw0 < rows ? row_lim(rw0) : -1;
  const int n_tiles = maxlim >= 0 ? maxlim / TP + 1 : 0;

  // this lane's query row
  const long long r = rw0 + l16;
  const int ti = (int)(r / G), g = (int)(r - (long long)ti * G);
  const long long tok = (long long)q0 + ti;
  const bool live = r < rows && tok >= 0 && tok < a.t;
  const int lim = live ? row_lim(r) : -1;
  const long long qrow = (tok * H + hkv * G + g) * D;

  // ---- staging: global -> registers -> LDS ---------------------------------
  uint4 kreg[NIT], vreg[NIT];
  float pk = 0.f, pv = 0.f;
  bool pok = false;
  // cached row of position pos for this block's kv head: element offset into
  // the code pools and into the scale pools; false: nothing to read
  auto locate = [&](int pos, long long& crow, long long& srow) -> bool {
    if (pos > maxlim) return false;
    const int phys = a.block_table[(long long)b * max_blocks + pos / bs];
    const int off = pos % bs;
    // a table entry outside the pool reads nothing
    if ((unsigned)phys >= (unsigned)a.nblocks) return false;
    crow = (long long)phys * a.cs_blk + (long long)off * a.cs_pos +
           (long long)hkv * a.cs_head;
    srow = (long long)phys * a.ss_blk + (long long)off * a.ss_pos +
           (long long)hkv * a.ss_head;
    return true;
  };
  auto load_tile = [&](int t) {
    const int p0 = t * TP;
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const int it = tid + 256 * k;
      const int ch = it % NCH;
      long long crow = 0, srow = 0;
      kreg[k] = make_uint4(0, 0, 0, 0);
      vreg[k] = kreg[k];
      if (locate(p0 + it / NCH, crow, srow)) {
        kreg[k] = *reinterpret_cast<const uint4*>(kcache + crow + ch * CW);
        vreg[k] = *reinterpret_cast<const uint4*>(vcache + crow + ch * CW);
      }
    }
    if (wid == 0) {
      long long crow = 0, srow = 0;
      pok = locate(p0 + lane, crow, srow);
      if constexpr (INT8) {
        pk = pok ? a.kscale[srow] * a.scale : 0.f;
        pv = pok ? a.vscale[srow] : 0.f;
      }
    }
  };
  auto store_image = [&](char* img, const uint4 (&reg)[NIT], bool is_v) {
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const int it = tid + 256 * k;
      const unsigned row = it / NCH, ch = it % NCH;
      const unsigned w[4] = {reg[k].x, reg[k].y, reg[k].z, reg[k].w};
      if constexpr (INT8) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const uint4 o = make_uint4(
              pf_codes2bf(w[2 * c], 0), pf_codes2bf(w[2 * c], 2),
              pf_codes2bf(w[2 * c + 1], 0), pf_codes2bf(w[2 * c + 1], 2));
          const unsigned off = is_v ? pf_off_v<D>(row, 2 * ch + c)
                                    : pf_off_k<D>(row, 2 * ch + c);
          *reinterpret_cast<uint4*>(img + off) = o;
        }
      } else {
        const unsigned off = is_v ? pf_off_v<D>(row, ch) : pf_off_k<D>(row, ch);
        *reinterpret_cast<uint4*>(img + off) = reg[k];
      }
    }
  };
  auto store_tile = [&]() {
    store_image(kimg, kreg, false);
    store_image(vimg, vreg, true);
    if (wid == 0) {
      const unsigned long long m = __ballot(pok);
      if (lane == 0) *okmask = m;
      if constexpr (INT8) {
        kmul[lane] = pk;
        vmul[lane] = pv;
      }
    }
  };

  if (n_tiles > 0) load_tile(0);

  // Q^T fragments: B[k = d][col = row], lane holds d = 32*ks + 8*hq + 0..7
  shortx8 qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    qf[ks] = shortx8{0, 0, 0, 0, 0, 0, 0, 0};
    if (live)
      qf[ks] = *reinterpret_cast<const shortx8*>((const short*)a.q + qrow +
                                                 32 * ks + 8 * hq);
  }

  floatx4 oacc[NDT];
#pragma unroll
  for (int n = 0; n < NDT; ++n) oacc[n] = floatx4{0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f;  // finite sentinel: -ffast-math breaks +-inf
  float l_run = 0.f;     // this lane's share of the row sum

  // LDS addresses of the lane's transposed reads, one per d tile: row
  // 4*hq + (l16 >> 2), 8 bytes at columns 16*n + 4*(l16 & 3)
  const unsigned lds_v =
      (unsigned)(size_t)(__attribute__((address_space(3))) char*)vimg;
  unsigned va[NDT];
#pragma unroll
  for (int n = 0; n < NDT; ++n)
    va[n] = lds_v + pf_off_v<D>(4 * hq + (l16 >> 2), 2 * n + ((l16 >> 1) & 1)) +
            8 * (l16 & 1);

  for (int t = 0; t < n_tiles; ++t) {
    const int p0 = t * TP;
    __syncthreads();                         // readers of the previous tile
    store_tile();
    __syncthreads();
    if (t + 1 < n_tiles) load_tile(t + 1);   // in flight under the math
    if (p0 > wmaxlim) continue;              // wave-uniform: above every row

    // ---- S^T = K Q^T ------------------------------------------------------
    floatx4 s[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      s[tt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const shortx8 kf = *reinterpret_cast<const shortx8*>(
            kimg + pf_off_k<D>(16 * tt + l16, 4 * ks + hq));
        s[tt] = mfma_bf16(kf, qf[ks], s[tt]);
      }
    }
    // ---- scale, mask, online softmax ---------------------------------------
    const uint2 okw = *reinterpret_cast<const uint2*>(okmask);
    const unsigned long long okm =
        ((unsigned long long)__builtin_amdgcn_readfirstlane(okw.y) << 32) |
        (unsigned)__builtin_amdgcn_readfirstlane(okw.x);
    // only tiles that touch the diagonal, S or an empty position mask
    const bool need_mask = p0 + TP - 1 > wminlim || okm != ~0ull;
    float mx = -1e30f;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      floatx4 km;
      if constexpr (INT8)
        km = *reinterpret_cast<const floatx4*>(kmul + 16 * tt + 4 * hq);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float x = s[tt][rr] * (INT8 ? km[rr] : a.scale);
        if (need_mask) {
          const int pl = 16 * tt + 4 * hq + rr;
          const bool vis = p0 + pl <= lim && ((okm >> pl) & 1ull);
          x = vis ? x : -1e30f;
        }
        s[tt][rr] = x;
        mx = fmaxf(mx, x);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
    const float m_new = fmaxf(m_run, mx);
    const float corr = __expf(m_run - m_new);  // 0 from the sentinel, or 1
    m_run = m_new;
    float psum = 0.f;
    shortx8 pf[2];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      floatx4 vm;
      if constexpr (INT8)
        vm = *reinterpret_cast<const floatx4*>(vmul + 16 * tt + 4 * hq);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float p = __expf(s[tt][rr] - m_new);
        if (need_mask) p = s[tt][rr] > -1e30f ? p : 0.f;
        psum += p;
        if constexpr (INT8) p *= vm[rr];
        pf[tt >> 1][4 * (tt & 1) + rr] = f2bf(p);
      }
    }
    l_run = l_run * corr + psum;
#pragma unroll
    for (int n = 0; n < NDT; ++n) oacc[n] *= corr;
    // ---- O^T += V^T P^T ------------------------------------------------------
#pragma unroll
    for (int n = 0; n < NDT; n += 4) {
      shortx8 vf[4];
      pf_tr_read4<0, 16 * RS>(vf, va[n], va[n + 1], va[n + 2], va[n + 3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) oacc[n + j] = mfma_bf16(vf[j], pf[0], oacc[n + j]);
      pf_tr_read4<32 * RS, 48 * RS>(vf, va[n], va[n + 1], va[n + 2], va[n + 3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) oacc[n + j] = mfma_bf16(vf[j], pf[1], oacc[n + j]);
    }
  }

  // ---- epilogue: lane holds O[row][16*n + 4*hq + 0..3] ------------------------
  l_run += __shfl_xor(l_run, 16, WAVE);
  l_run += __shfl_xor(l_run, 32, WAVE);
  if (!live) return;
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;  // nothing visible: zeros
  short* op = (short*)a.o + qrow + 4 * hq;
#pragma unroll
  for (int n = 0; n < NDT; ++n) {
    shortx4 o4;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) o4[rr] = f2bf(oacc[n][rr] * inv);
    *reinterpret_cast<shortx4*>(op + 16 * n) = o4;
  }
}

}  // namespace

void paged_prefill_attention(const PrefillAttnArgs& a, hipStream_t s) {
  if (a.t == 0 || a.b == 0) return;
  const long long rows = (long long)a.max_q * (a.h / a.hkv);
  const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)a.hkv, (unsigned)a.b);
#define PA_PF_LAUNCH(DH, I8)                                                  \
  hipLaunchKernelGGL((paged_prefill_kernel<DH, I8>), grid, dim3(256), 0, s, a)
  if (a.kscale != nullptr) {
    if (a.dh == 128) PA_PF_LAUNCH(128, true); else PA_PF_LAUNCH(64, true);
  } else {
    if (a.dh == 128) PA_PF_LAUNCH(128, false); else PA_PF_LAUNCH(64, false);
  }
#undef PA_PF_LAUNCH
}

}  // namespace pa
