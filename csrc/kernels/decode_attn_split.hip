// Split-KV paged decode attention for gfx950 (docs/KERNELS.md "split-KV
// decode attention").
//
// decode_attn.hip gives one block to each (sequence, q-head): at low batch a
// handful of CUs walk the whole context serially, and with GQA the G = H/HKV
// blocks of a group fetch the same K/V rows.  Here a block owns
// (split s, head tile, kv head, sequence b):
//   * a tile of GT consecutive q-heads of one kv head's group shares each
//     K/V register load (qv/oacc/m/l per head), so rows are fetched once
//     per tile instead of once per q-head;
//   * the positions of a sequence are cut into nsplit slices by a rule
//     evaluated on the device from seq_lens, so captured graphs stay valid;
//   * partials (max, sum, unnormalised o) go to fp32 workspaces with plain
//     vector stores, and decode_attn_merge_kernel combines them in a fixed
//     order -- no atomics, no cross-workgroup flags, same bits every run.
// Lane layout per position as in decode_attn.hip: bf16 cache 16 lanes x
// D/16 elements (16 positions per block step), int8 cache D/16 lanes x 16
// codes (32 | 64 positions per block step); next step's loads are issued
// before this step's math; finite -1e30 sentinel.
#include "common.h"
#include "api.h"

namespace pa {

namespace {

// byte i of w, sign-extended, as float (see decode_attn.hip)
__device__ __forceinline__ float code2f_s(unsigned w, int i) {
  return (float)(int)(signed char)(w >> (8 * i));
}

template <int LANES>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1)
    v += __shfl_xor(v, off, WAVE);
  return v;
}

}  // namespace

template <int D, int GT, bool INT8>
__launch_bounds__(256)
__global__ void decode_attn_split_kernel(
    const short* __restrict__ qg, const void* __restrict__ kcache_v,
    const void* __restrict__ vcache_v, const float* __restrict__ kscale,
    const float* __restrict__ vscale, const int* __restrict__ block_table,
    const int* __restrict__ seq_lens, float* __restrict__ o_part,
    float* __restrict__ ml_part, int H, int HKV, int bs, int max_blocks,
    int nblocks, int nsplit, int tiles, float scale, long long ss_blk,
    long long ss_pos, long long ss_head) {
  constexpr int E = INT8 ? 16 : D / 16;     // elements per lane
  constexpr int LPP = D / E;                // lanes per position
  constexpr int PPW = 64 / LPP;             // positions per wave step
  constexpr int SLOTS = 4 * PPW;            // positions per block step
  static_assert(64 % SLOTS == 0, "slice granule 64 covers whole block steps");

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

  // slice rule (part of the contract): never walk past the table
  const int S = max(0, min(seq_lens[b], max_blocks * bs));
  const int c = 64 * ((S + 64 * nsplit - 1) / (64 * nsplit));
  const int begin = s * c;
  const int end = min(S, begin + c);

  const long long row0 = ((long long)b * H + h0) * nsplit + s;  // + g * nsplit
  if (begin >= end) {                       // empty slice: l = 0, m = -1e30
    for (int g = 0; g < nh; ++g) {
      const long long r = row0 + (long long)g * nsplit;
      if (tid < D) o_part[r * D + tid] = 0.f;
      if (tid == 0)
        *reinterpret_cast<float2*>(ml_part + r * 2) = make_float2(-1e30f, 0.f);
    }
    return;
  }

  // q of the tile's heads, softmax scale folded in; a surplus head is zero
  // and its q is never read
  float qv[GT][E];
#pragma unroll
  for (int g = 0; g < GT; ++g) {
#pragma unroll
    for (int i = 0; i < E; ++i) qv[g][i] = 0.f;
    if (g < nh) {
      const short* qp = qg + ((long long)b * H + h0 + g) * D + lg * E;
      if constexpr (E == 4) {
        const shortx4 q4 = *reinterpret_cast<const shortx4*>(qp);
#pragma unroll
        for (int i = 0; i < 4; ++i) qv[g][i] = bf2f(q4[i]) * scale;
      } else {
#pragma unroll
        for (int j = 0; j < E; j += 8) {
          const shortx8 q8 = *reinterpret_cast<const shortx8*>(qp + j);
#pragma unroll
          for (int i = 0; i < 8; ++i) qv[g][j + i] = bf2f(q8[i]) * scale;
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
      ok = (unsigned)phys < (unsigned)nblocks;
      if (ok) {
        const long long row = ((long long)phys * bs + off) * HKV + hkv;
        if constexpr (INT8) {
          const signed char* kc = (const signed char*)kcache_v;
          const signed char* vc = (const signed char*)vcache_v;
          const long long srow = (long long)phys * ss_blk +
                                 (long long)off * ss_pos +
                                 (long long)hkv * ss_head;
          kw = *reinterpret_cast<const uint4*>(kc + row * D + lg * 16);
          vw = *reinterpret_cast<const uint4*>(vc + row * D + lg * 16);
          dk = kscale[srow];
          dv = vscale[srow];
        } else {
          const short* kc = (const short*)kcache_v + row * D + lg * E;
          const short* vc = (const short*)vcache_v + row * D + lg * E;
          if constexpr (E == 8) {
            kw = *reinterpret_cast<const uint4*>(kc);
            vw = *reinterpret_cast<const uint4*>(vc);
          } else {
            const uint2 k2 = *reinterpret_cast<const uint2*>(kc);
            const uint2 v2 = *reinterpret_cast<const uint2*>(vc);
            kw.x = k2.x; kw.y = k2.y;
            vw.x = v2.x; vw.y = v2.y;
          }
        }
      }
    }
  };
  // element i of a loaded register quad as float
  auto elem = [](const unsigned (&w)[4], int i) -> float {
    if constexpr (INT8) {
      return code2f_s(w[i >> 2], i & 3);
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
  for (int pos0 = p_start; pos0 < end; pos0 += SLOTS) {
    if (pos0 + SLOTS < end) load_kv(pos0 + SLOTS, okn, kn, vn, dkn, dvn);
    else okn = false;
    const bool ok = okc;
    const unsigned kwd[4] = {kc.x, kc.y, kc.z, kc.w};
    const unsigned vwd[4] = {vc.x, vc.y, vc.z, vc.w};
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
      sc = group_sum<LPP>(sc);
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
      const float vf = ok ? elem(vwd, i) : 0.f;
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
      const long long r = row0 + (long long)g * nsplit;
      o_part[r * D + tid] = out;
      if (tid == 0)
        *reinterpret_cast<float2*>(ml_part + r * 2) = make_float2(gm, gl);
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

void decode_attention_split(const void* q, const void* kcache,
                            const void* vcache, const float* kscale,
                            const float* vscale, const int* block_table,
                            const int* seq_lens, void* o, float* o_part,
                            float* ml_part, int64_t b, int64_t h, int64_t hkv,
                            int64_t bs, int64_t max_blocks, int64_t nblocks,
                            int64_t dh, float scale, int64_t nsplit,
                            int64_t ss_blk, int64_t ss_pos, int64_t ss_head,
                            hipStream_t s) {
  if (b * h == 0) return;
  const bool int8 = kscale != nullptr;
  const DecodeAttnSplitPlan plan =
      decode_attn_split_plan(b, h, hkv, nsplit, int8);
  const dim3 grid((unsigned)plan.blocks);
#define PA_DAS_LAUNCH(DH, GT, I8)                                             \
  hipLaunchKernelGGL((decode_attn_split_kernel<DH, GT, I8>), grid, dim3(256), \
                     0, s, (const short*)q, kcache, vcache, kscale, vscale,   \
                     block_table, seq_lens, o_part, ml_part, (int)h,          \
                     (int)hkv, (int)bs, (int)max_blocks, (int)nblocks,        \
                     (int)nsplit, plan.tiles, scale, (long long)ss_blk,       \
                     (long long)ss_pos, (long long)ss_head)
  // GT = 8 exists for the bf16 cache only (the plan never asks int8 for it)
#define PA_DAS_GT(DH, I8, GTMAX)                                              \
  switch (plan.gt) {                                                          \
    case 1: PA_DAS_LAUNCH(DH, 1, I8); break;                                  \
    case 2: PA_DAS_LAUNCH(DH, 2, I8); break;                                  \
    case 4: PA_DAS_LAUNCH(DH, 4, I8); break;                                  \
    default: PA_DAS_LAUNCH(DH, GTMAX, I8); break;                             \
  }
  if (int8) {
    if (dh == 128) { PA_DAS_GT(128, true, 4) } else { PA_DAS_GT(64, true, 4) }
  } else {
    if (dh == 128) { PA_DAS_GT(128, false, 8) } else { PA_DAS_GT(64, false, 8) }
  }
#undef PA_DAS_GT
#undef PA_DAS_LAUNCH
  const long long rows = b * h;
  const dim3 mgrid((unsigned)((rows + 3) / 4));
  if (dh == 128)
    hipLaunchKernelGGL((decode_attn_merge_kernel<128>), mgrid, dim3(256), 0, s,
                       o_part, ml_part, (short*)o, rows, (int)nsplit);
  else
    hipLaunchKernelGGL((decode_attn_merge_kernel<64>), mgrid, dim3(256), 0, s,
                       o_part, ml_part, (short*)o, rows, (int)nsplit);
}

}  // namespace pa
