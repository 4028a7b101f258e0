// Paged-KV single-token decode attention for gfx950 (serving path;
// docs/KERNELS.md "paged decode attention") and the int8 KV cache's
// quantize-on-append.
//
// Reference role parity: paddle/phi/kernels/fusion/gpu/
// masked_multihead_attention_kernel.cu + block_multi_head_attention
// (paged "block" KV cache) -- re-derived for wave64.
//
// One kernel template serves the bf16 and int8 caches, the paged and the
// dense layout, unsplit and split-KV.  A 256-thread block owns
// (split s, head tile, kv head, sequence b):
//   * a tile of GT consecutive q-heads of one kv head's group shares each
//     K/V register load (qv/oacc/m/l per head), so rows are fetched once
//     per tile instead of once per q-head;
//   * PARTIAL: the positions of a sequence are cut into nsplit slices by a
//     rule evaluated on the device from seq_lens, so captured graphs stay
//     valid; partials (max, sum, unnormalised o) go to fp32 workspaces with
//     plain vector stores, and decode_attn_merge_kernel combines them in a
//     fixed order -- no atomics, no cross-workgroup flags, same bits every
//     run;
//   * !PARTIAL: the block walks [0, S) and writes bf16 o itself.
// Lane layout per position: bf16 cache 16 lanes x D/16 elements (16
// positions per block step), int8 cache D/16 lanes x 16 codes (32 | 64
// positions per block step), 16 B per lane in flight (8 B at bf16 D = 64);
// next step's loads are issued before this step's math; online softmax in
// registers with a finite -1e30 sentinel; the block's position slots merge
// through LDS in slot order.
#include <type_traits>

#include "common.h"
#include "api.h"

namespace pa {

// ===========================================================================
// int8 paged KV cache (docs/KERNELS.md "int8 KV cache")
//   codes  int8 [nblocks, bs, HKV, D], two's complement in [-127, 127]
//   scales fp32, addressed (blk, pos, head) by element strides:
//     per token  [nblocks, bs, HKV] -> (bs*HKV, HKV, 1)
//     per head   [HKV]              -> (0, 0, 1)
//   x^ = code * scale
// ===========================================================================

// byte i of w, sign-extended, as float: one v_cvt_f32_i32 with an SDWA
// sext(BYTE_i) source on gfx950.  The 16 codes of a lane stay in a uint4 --
// a vector of i8 is legalised to one VGPR per byte.
__device__ __forceinline__ float code2f(unsigned w, int i) {
  return (float)(int)(signed char)(w >> (8 * i));
}

template <int LANES, typename Op>
__device__ __forceinline__ float group_reduce(float v, Op op) {
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1)
    v = op(v, __shfl_xor(v, off, WAVE));
  return v;
}

__device__ __forceinline__ unsigned quant_byte(float x, float inv) {
  float r = fminf(fmaxf(rintf(x * inv), -127.f), 127.f);
  return (unsigned)(int)r & 0xffu;
}

// One D/8-lane group per (token, kv head) row, 8 bf16 per lane (16 B load,
// 8 B store).  blockIdx.y: 0 = K, 1 = V.  qs == nullptr: per-token mode,
// d = absmax * fp32(1/127) is written to the scale pool; else fixed mode,
// code = rint(x * qs[h]) and no scale is written.  Rows whose (blk, off)
// fall outside the pool are skipped.
template <int D>
__launch_bounds__(256)
__global__ void kv_quant_append_kernel(
    const short* __restrict__ kg, const short* __restrict__ vg,
    signed char* __restrict__ kcache, signed char* __restrict__ vcache,
    float* __restrict__ kscale, float* __restrict__ vscale,
    const long long* __restrict__ blk, const long long* __restrict__ off,
    const float* __restrict__ kqs, const float* __restrict__ vqs,
    long long rows, int HKV, int bs, long long nblocks,
    long long k_tstr, long long k_hstr, long long v_tstr, long long v_hstr) {
  constexpr int LPR = D / 8;             // lanes per row: 16 | 8
  constexpr int RPB = 256 / LPR;         // rows per block
  const bool is_v = blockIdx.y != 0;
  const long long r = (long long)blockIdx.x * RPB + threadIdx.x / LPR;
  if (r >= rows) return;                 // whole lane groups leave together
  const int lg = threadIdx.x % LPR;
  const long long t = r / HKV;
  const int h = (int)(r % HKV);
  const short* src = is_v ? vg + t * v_tstr + h * v_hstr
                          : kg + t * k_tstr + h * k_hstr;
  const shortx8 x8 = *reinterpret_cast<const shortx8*>(src + lg * 8);
  float x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = bf2f(x8[i]);

  const float* qs = is_v ? vqs : kqs;
  float d = 0.f, inv;
  if (qs == nullptr) {
    float am = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(x[i]));
    am = group_reduce<LPR>(am, MaxOp());
    d = am * (1.0f / 127.0f);            // one fp32 multiply by fp32(1/127)
    inv = d > 0.f ? 1.0f / d : 0.f;      // zero row: codes 0, no division
  } else {
    inv = qs[h];
  }
  unsigned w0 = 0, w1 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w0 |= quant_byte(x[i], inv) << (8 * i);
    w1 |= quant_byte(x[4 + i], inv) << (8 * i);
  }
  const long long pb = blk[t], po = off[t];
  if (pb < 0 || pb >= nblocks || po < 0 || po >= bs) return;
  const long long row = (pb * bs + po) * HKV + h;
  uint2 w = make_uint2(w0, w1);
  *reinterpret_cast<uint2*>((is_v ? vcache : kcache) + row * D + lg * 8) = w;
  if (qs == nullptr && lg == 0) (is_v ? vscale : kscale)[row] = d;
}

void kv_quant_append(const void* k, const void* v, void* kcache, void* vcache,
                     float* kscale, float* vscale, const int64_t* blk,
                     const int64_t* off, const float* k_qscale,
                     const float* v_qscale, int64_t t, int64_t hkv, int64_t dh,
                     int64_t bs, int64_t nblocks, int64_t k_tstr,
                     int64_t k_hstr, int64_t v_tstr, int64_t v_hstr,
                     hipStream_t s) {
  const long long rows = t * hkv;
  if (rows == 0) return;
  const int rpb = 256 / (int)(dh / 8);
  dim3 grid((unsigned)((rows + rpb - 1) / rpb), 2);
#define PA_KVQ_LAUNCH(DH)                                                     \
  hipLaunchKernelGGL((kv_quant_append_kernel<DH>), grid, dim3(256), 0, s,     \
                     (const short*)k, (const short*)v, (signed char*)kcache,  \
                     (signed char*)vcache, kscale, vscale,                    \
                     (const long long*)blk, (const long long*)off, k_qscale,  \
                     v_qscale, rows, (int)hkv, (int)bs, (long long)nblocks,   \
                     (long long)k_tstr, (long long)k_hstr, (long long)v_tstr, \
                     (long long)v_hstr)
  if (dh == 128) PA_KVQ_LAUNCH(128);
  else PA_KVQ_LAUNCH(64);
#undef PA_KVQ_LAUNCH
}

// ===========================================================================
// decode attention
// ===========================================================================
// int8 scales act on the result, not on the element: the softmax scale is
// folded into q, score = (sum q_i code_i) * d_k[pos],
// oacc += (p * d_v[pos]) * code.
template <int D, int GT, bool INT8, bool PARTIAL>
__launch_bounds__(256)
__global__ void decode_attn_kernel(const DecodeAttnArgs a, const int tiles) {
  constexpr int E = INT8 ? 16 : D / 16;     // elements per lane
  constexpr int LPP = D / E;                // lanes per position
  constexpr int PPW = 64 / LPP;             // positions per wave step
  constexpr int SLOTS = 4 * PPW;            // positions per block step
  static_assert(64 % SLOTS == 0, "slice granule 64 covers whole block steps");
  using cache_t = std::conditional_t<INT8, signed char, short>;
  const cache_t* __restrict__ kcache = (const cache_t*)a.kcache;
  const cache_t* __restrict__ vcache = (const cache_t*)a.vcache;
  const int* __restrict__ block_table = a.block_table;
  const int H = a.h, HKV = a.hkv, bs = a.bs, max_blocks = a.max_blocks;
  const int nsplit = PARTIAL ? a.nsplit : 1;

  int idx = blockIdx.x;
  const int s = idx % nsplit; idx /= nsplit;
  const int tile = idx % tiles; idx /= tiles;
  const int hkv = idx % HKV;
  const int b = idx / HKV;
  const int G = H / HKV;
  const int h0 = hkv * G + tile * GT;       // first q-head of the tile
  const int nh = min(GT, G - tile * GT);    // live heads; surplus is guarded

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int lg = lane % LPP;                // element group within D
  const int lp = lane / LPP;                // position slot within the wave

  // never walk past the table; PARTIAL: the slice rule (part of the contract)
  const int S = max(0, min(a.seq_lens[b], max_blocks * bs));
  int begin = 0, end = S;
  if constexpr (PARTIAL) {
    const int c = 64 * ((S + 64 * nsplit - 1) / (64 * nsplit));
    begin = s * c;
    end = min(S, begin + c);
  }

  // Result of head g of the tile, called by the thread tid < D that owns
  // column tid: the partial (out, gm, gl), or the normalised bf16 output.
  const long long row0 = ((long long)b * H + h0) * nsplit + s;  // + g * nsplit
  auto store = [&](int g, float out, float gm, float gl) {
    const long long r = row0 + (long long)g * nsplit;
    if constexpr (PARTIAL) {
      a.o_part[r * D + tid] = out;
      if (tid == 0)
        *reinterpret_cast<float2*>(a.ml_part + r * 2) = make_float2(gm, gl);
    } else {
      ((short*)a.o)[r * D + tid] = f2bf(out * (gl > 0.f ? 1.f / gl : 0.f));
    }
  };
  if (begin >= end) {                       // nothing to read: l = 0, m = -1e30
    if (tid < D)
      for (int g = 0; g < nh; ++g) store(g, 0.f, -1e30f, 0.f);
    return;
  }

  // One position's K and V for this lane: 16 B each (8 B at bf16 D = 64),
  // plus d_k / d_v of the int8 cache in the same prefetch stage.
  auto load_kv = [&](int pos0, bool& ok, uint4& kw, uint4& vw, float& dk,
                     float& dv) {
    const int pos = pos0 + lp;
    ok = pos < end;
    if (ok) {
      const int phys = block_table[(long long)b * max_blocks + pos / bs];
      const int off = pos % bs;
      // a table entry outside the pool reads nothing (wrong numbers, no fault)
      ok = (unsigned)phys < (unsigned)a.nblocks;
      if (ok) {
        const long long row = (long long)phys * a.cs_blk +
                              (long long)off * a.cs_pos +
                              (long long)hkv * a.cs_head + lg * E;
        if constexpr (E == 4) {
          const uint2 k2 = *reinterpret_cast<const uint2*>(kcache + row);
          const uint2 v2 = *reinterpret_cast<const uint2*>(vcache + row);
          kw.x = k2.x; kw.y = k2.y;
          vw.x = v2.x; vw.y = v2.y;
        } else {
          kw = *reinterpret_cast<const uint4*>(kcache + row);
          vw = *reinterpret_cast<const uint4*>(vcache + row);
        }
        if constexpr (INT8) {
          const long long srow = (long long)phys * a.ss_blk +
                                 (long long)off * a.ss_pos +
                                 (long long)hkv * a.ss_head;
          dk = a.kscale[srow];
          dv = a.vscale[srow];
        }
      }
    }
  };
  // element i of a loaded register quad as float
  auto elem = [](const unsigned (&w)[4], int i) -> float {
    if constexpr (INT8) {
      return code2f(w[i >> 2], i & 3);
    } else {
      const unsigned u = w[i >> 1];
      return __uint_as_float((i & 1) ? (u & 0xffff0000u) : (u << 16));
    }
  };

  bool okc = false, okn = false;
  uint4 kc = make_uint4(0, 0, 0, 0), vc = kc, kn = kc, vn = kc;
  float dkc = 1.f, dvc = 1.f, dkn = 1.f, dvn = 1.f;
  const int p_start = begin + wid * PPW;
  load_kv(p_start, okc, kc, vc, dkc, dvc);

  // q of the tile's heads, softmax scale folded in; a surplus head is zero
  // and its q is never read.  Loaded after the first K/V so that the two
  // latencies overlap.
  float qv[GT][E];
#pragma unroll
  for (int g = 0; g < GT; ++g) {
#pragma unroll
    for (int i = 0; i < E; ++i) qv[g][i] = 0.f;
    if (g < nh) {
      const short* qp =
          (const short*)a.q + ((long long)b * H + h0 + g) * D + lg * E;
      if constexpr (E == 4) {
        const shortx4 q4 = *reinterpret_cast<const shortx4*>(qp);
#pragma unroll
        for (int i = 0; i < 4; ++i) qv[g][i] = bf2f(q4[i]) * a.scale;
      } else {
#pragma unroll
        for (int j = 0; j < E; j += 8) {
          const shortx8 q8 = *reinterpret_cast<const shortx8*>(qp + j);
#pragma unroll
          for (int i = 0; i < 8; ++i) qv[g][j + i] = bf2f(q8[i]) * a.scale;
        }
      }
    }
  }

  float m[GT], l[GT], oacc[GT][E];
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    m[g] = -1e30f;  // finite sentinel: -ffast-math breaks +-inf
    l[g] = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) oacc[g][i] = 0.f;
  }

  // s_waitcnt vmcnt(0): the first loads land before the loop.  Left pending
  // across the loop header, they make the compiler wait inside every step
  // right after the prefetch is issued (for the prefetch's own first load),
  // which serialises load latency and math; with this the step waits only
  // where it rotates the registers, at its end.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  for (int pos0 = p_start; pos0 < end; pos0 += SLOTS) {
    if (pos0 + SLOTS < end) load_kv(pos0 + SLOTS, okn, kn, vn, dkn, dvn);
    else okn = false;
    const bool ok = okc;
    const unsigned kwd[4] = {kc.x, kc.y, kc.z, kc.w};
    // p = 0 masks a position: enough for codes, which are finite; stale bf16
    // bits are zeroed a word at a time
    const bool vlive = INT8 || ok;
    const unsigned vwd[4] = {vlive ? vc.x : 0u, vlive ? vc.y : 0u,
                             vlive ? vc.z : 0u, vlive ? vc.w : 0u};
    // K of this position, decoded once for the GT heads
    float kf[E];
#pragma unroll
    for (int i = 0; i < E; ++i) kf[i] = elem(kwd, i);
    float p[GT], corr[GT];
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      float sc = 0.f;
#pragma unroll
      for (int i = 0; i < E; ++i) sc += qv[g][i] * kf[i];
      sc = group_reduce<LPP>(sc, SumOp());
      if constexpr (INT8) sc *= dkc;
      sc = ok ? sc : -1e30f;
      const float m_new = fmaxf(m[g], sc);
      corr[g] = __expf(m[g] - m_new);     // underflows to 0 for the sentinel
      const float pg = ok ? __expf(sc - m_new) : 0.f;
      l[g] = l[g] * corr[g] + pg;
      m[g] = m_new;
      if constexpr (INT8) p[g] = ok ? pg * dvc : 0.f;
      else p[g] = pg;
    }
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const float vf = elem(vwd, i);
#pragma unroll
      for (int g = 0; g < GT; ++g)
        oacc[g][i] = oacc[g][i] * corr[g] + p[g] * vf;
    }
    okc = okn; kc = kn; vc = vn; dkc = dkn; dvc = dvn;
  }

  // ---- in-block merge of the SLOTS position-slot partials, head by head ---
  // One LDS image reused for every head of the tile; thread `tid < D` owns
  // one output column and walks the slots in fixed order.
  __shared__ float sm[SLOTS], sl[SLOTS];
  __shared__ __attribute__((aligned(16))) float so[SLOTS][D];
  const int slot_id = wid * PPW + lp;
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    if (g >= nh) break;                     // block-uniform
    if (g > 0) __syncthreads();             // readers of the previous head
    if (lg == 0) {
      sm[slot_id] = m[g];
      sl[slot_id] = l[g];
    }
#pragma unroll
    for (int i = 0; i < E; i += 4) {
      const floatx4 o4 = {oacc[g][i], oacc[g][i + 1], oacc[g][i + 2],
                          oacc[g][i + 3]};
      *reinterpret_cast<floatx4*>(&so[slot_id][lg * E + i]) = o4;
    }
    __syncthreads();
    if (tid < D) {
      float gm = -1e30f;
#pragma unroll
      for (int s2 = 0; s2 < SLOTS; ++s2) gm = fmaxf(gm, sm[s2]);
      float gl = 0.f, out = 0.f;
#pragma unroll 8
      for (int s2 = 0; s2 < SLOTS; ++s2) {
        const float w = (sl[s2] > 0.f) ? __expf(sm[s2] - gm) : 0.f;
        gl += sl[s2] * w;
        out += w * so[s2][tid];
      }
      store(g, out, gm, gl);
    }
  }
}

// One wave per (b, h) row, 4 rows per block; lane owns D/64 output elements.
// Splits combine in index order: gm = max m_s, w_s = l_s > 0 ? exp(m_s - gm)
// : 0, out = sum w_s o_s / sum w_s l_s.  A row with no live split is zero.
template <int D>
__launch_bounds__(256)
__global__ void decode_attn_merge_kernel(const float* __restrict__ o_part,
                                         const float* __restrict__ ml_part,
                                         short* __restrict__ og,
                                         long long rows, int nsplit) {
  constexpr int EPL = D / 64;
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                    // whole waves leave together
  const float* ml = ml_part + r * nsplit * 2;
  const float* op = o_part + r * nsplit * D + lane * EPL;
  float gm = -1e30f;
  for (int s = 0; s < nsplit; ++s) gm = fmaxf(gm, ml[2 * s]);
  float gl = 0.f, out[EPL];
#pragma unroll
  for (int i = 0; i < EPL; ++i) out[i] = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float ls = ml[2 * s + 1];
    const float w = ls > 0.f ? __expf(ml[2 * s] - gm) : 0.f;
    gl += w * ls;
#pragma unroll
    for (int i = 0; i < EPL; ++i) out[i] += w * op[(long long)s * D + i];
  }
  const float inv = gl > 0.f ? 1.f / gl : 0.f;   // S == 0 -> zeros
#pragma unroll
  for (int i = 0; i < EPL; ++i) og[r * D + lane * EPL + i] = f2bf(out[i] * inv);
}

DecodeAttnSplitPlan decode_attn_split_plan(int64_t b, int64_t h, int64_t hkv,
                                           int64_t nsplit, bool int8) {
  const int64_t g = hkv > 0 ? h / hkv : 1;
  const int gmax = int8 ? 4 : 8;
  int gt = 1;
  while (gt < g && gt < gmax) gt *= 2;
  const int tiles = (int)((g + gt - 1) / gt);
  return {gt, tiles, b * hkv * tiles * nsplit};
}

void decode_attention(const DecodeAttnArgs& a, hipStream_t s) {
  if ((int64_t)a.b * a.h == 0) return;
  const bool int8 = a.kscale != nullptr, partial = a.nsplit > 0;
  const DecodeAttnSplitPlan plan =
      partial ? decode_attn_split_plan(a.b, a.h, a.hkv, a.nsplit, int8)
              : DecodeAttnSplitPlan{1, a.h / a.hkv, (int64_t)a.b * a.h};
  const dim3 grid((unsigned)plan.blocks);
#define PA_DA_LAUNCH(DH, GT, I8, P)                                           \
  hipLaunchKernelGGL((decode_attn_kernel<DH, GT, I8, P>), grid, dim3(256), 0, \
                     s, a, plan.tiles)
  // unsplit: GT = 1; GT = 8 exists for the bf16 cache only (the plan never
  // asks int8 for it)
#define PA_DA_GT(DH, I8, GTMAX)                                               \
  if (!partial) PA_DA_LAUNCH(DH, 1, I8, false);                               \
  else switch (plan.gt) {                                                     \
    case 1: PA_DA_LAUNCH(DH, 1, I8, true); break;                             \
    case 2: PA_DA_LAUNCH(DH, 2, I8, true); break;                             \
    case 4: PA_DA_LAUNCH(DH, 4, I8, true); break;                             \
    default: PA_DA_LAUNCH(DH, GTMAX, I8, true); break;                        \
  }
  if (int8) {
    if (a.dh == 128) { PA_DA_GT(128, true, 4) } else { PA_DA_GT(64, true, 4) }
  } else {
    if (a.dh == 128) { PA_DA_GT(128, false, 8) } else { PA_DA_GT(64, false, 8) }
  }
#undef PA_DA_GT
#undef PA_DA_LAUNCH
  if (!partial) return;
  const long long rows = (long long)a.b * a.h;
  const dim3 mgrid((unsigned)((rows + 3) / 4));
  if (a.dh == 128)
    hipLaunchKernelGGL((decode_attn_merge_kernel<128>), mgrid, dim3(256), 0, s,
                       a.o_part, a.ml_part, (short*)a.o, rows, a.nsplit);
  else
    hipLaunchKernelGGL((decode_attn_merge_kernel<64>), mgrid, dim3(256), 0, s,
                       a.o_part, a.ml_part, (short*)a.o, rows, a.nsplit);
}

}  // namespace pa
