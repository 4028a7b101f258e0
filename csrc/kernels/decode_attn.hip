// Paged-KV single-token decode attention for gfx950 (serving path).
//
// Reference role parity: paddle/phi/kernels/fusion/gpu/
// masked_multihead_attention_kernel.cu + block_multi_head_attention
// (paged "block" KV cache) -- re-derived for wave64:
//   * one 256-thread block per (batch, q-head); GQA via head mapping
//   * KV streamed from a paged cache: k/v_cache [nblocks, bs, hkv, D],
//     block_table [B, max_blocks] -- HBM-bound, 16B/lane loads
//   * 16 lanes per position (D<=128: 8 elems/lane), 4 pos/wave/step,
//     online softmax in registers, cross-wave merge via LDS
#include "common.h"
#include "api.h"

namespace pa {

template <int D>
__launch_bounds__(256)
__global__ void decode_attn_kernel(const short* __restrict__ qg,
                                   const short* __restrict__ kcache,
                                   const short* __restrict__ vcache,
                                   const int* __restrict__ block_table,
                                   const int* __restrict__ seq_lens,
                                   short* __restrict__ og,
                                   int B, int H, int HKV, int bs,
                                   int max_blocks, float scale,
                                   long long blk_str, long long pos_str,
                                   long long head_str) {
  const int b = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const int hkv = h / (H / HKV);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int l16 = lane & 15;   // element group within D
  const int lp = lane >> 4;    // 0..3: position slot within wave
  const int S = seq_lens[b];

  // q for this (b,h): D elems; 16-lane group covers D -> E = D/16 per lane
  constexpr int E = D / 16;
  float qv[E];
  {
    const short* qp = qg + ((long long)b * H + h) * D;
#pragma unroll
    for (int i = 0; i < E; ++i) qv[i] = bf2f(qp[l16 * E + i]);
  }

  float m = -1e30f, l = 0.f;  // finite sentinel: -ffast-math breaks +-inf
  float oacc[E];
#pragma unroll
  for (int i = 0; i < E; ++i) oacc[i] = 0.f;

  // each wave processes 4 positions per step; 4 waves -> 16 pos/block/step.
  // Software-pipelined: K/V for step t+1 load while step t computes --
  // the serial position walk was latency-bound (back-to-back dependent
  // 16 B loads per step).
  auto load_kv = [&](int pos0, bool& ok, shortx8& kv8, shortx8& vv8) {
    int pos = pos0 + lp;
    ok = pos < S;
    int phys = 0, off = 0;
    if (ok) {
      phys = block_table[(long long)b * max_blocks + pos / bs];
      off = pos % bs;
    }
    const long long base = (long long)phys * blk_str +
                           (long long)off * pos_str +
                           (long long)hkv * head_str + l16 * E;
    if (ok) {
      if (E == 8) {
        kv8 = *reinterpret_cast<const shortx8*>(kcache + base);
        vv8 = *reinterpret_cast<const shortx8*>(vcache + base);
      } else {
        shortx4 k4 = *reinterpret_cast<const shortx4*>(kcache + base);
        shortx4 v4 = *reinterpret_cast<const shortx4*>(vcache + base);
#pragma unroll
        for (int i = 0; i < 4; ++i) { kv8[i] = k4[i]; vv8[i] = v4[i]; }
      }
    }
  };

  bool okc = false, okn = false;
  shortx8 kc8, vc8, kn8, vn8;
  const int p_start = wid * 4;
  load_kv(p_start, okc, kc8, vc8);
  for (int pos0 = p_start; pos0 < S; pos0 += 16) {
    if (pos0 + 16 < S) load_kv(pos0 + 16, okn, kn8, vn8);
    else okn = false;
    bool ok = okc;
    float sc = 0.f;
    if (ok) {
#pragma unroll
      for (int i = 0; i < E; ++i) sc += qv[i] * bf2f(kc8[i]);
    }
    // reduce over the 16-lane group
    sc = group16_reduce(sc, SumOp());
    sc = ok ? sc * scale : -1e30f;
    // online softmax across the 4 position-slots handled by this wave-step
    float m_new = fmaxf(m, sc);
    float corr = __expf(m - m_new);       // underflows to 0 for the sentinel
    float p = ok ? __expf(sc - m_new) : 0.f;
    l = l * corr + p;
    m = m_new;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      float vvf = ok ? bf2f(vc8[i]) : 0.f;
      oacc[i] = oacc[i] * corr + p * vvf;
    }
    okc = okn; kc8 = kn8; vc8 = vn8;
  }

  // ---- merge the 16 position-slot partials (4 waves x 4 slots) ----------
  // each (wid, lp) slot has (m, l, oacc[8]) per l16 group
  __shared__ float sm[16], sl[16];
  __shared__ float so[16][D];
  const int slot_id = wid * 4 + lp;
  if (l16 == 0) {
    sm[slot_id] = m;
    sl[slot_id] = l;
  }
#pragma unroll
  for (int i = 0; i < E; ++i) so[slot_id][l16 * E + i] = oacc[i];
  __syncthreads();
  if (tid < 64) {
    // wave 0 merges 16 slots
    float gm = -1e30f;
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) gm = fmaxf(gm, sm[s2]);
    float gl = 0.f;
    float out[E];
#pragma unroll
    for (int i = 0; i < E; ++i) out[i] = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) {
      float w = (sl[s2] > 0.f) ? __expf(sm[s2] - gm) : 0.f;
      gl += sl[s2] * w;
#pragma unroll
      for (int i = 0; i < E; ++i) out[i] += w * so[s2][l16 * E + i];
    }
    if (lane < 16) {
      float inv = gl > 0.f ? 1.f / gl : 0.f;
      short* op = og + ((long long)b * H + h) * D;
#pragma unroll
      for (int i = 0; i < E; ++i) op[l16 * E + i] = f2bf(out[i] * inv);
    }
  }
}

void decode_attention(const void* q, const void* kcache, const void* vcache,
                      const int* block_table, const int* seq_lens, void* o,
                      int64_t b, int64_t h, int64_t hkv, int64_t bs,
                      int64_t max_blocks, int64_t dh, float scale,
                      int64_t blk_str, int64_t pos_str, int64_t head_str,
                      hipStream_t s) {
  dim3 grid((unsigned)(b * h));
  if (blk_str == 0) {   // default paged layout [nblocks, bs, HKV, D]
    blk_str = bs * hkv * dh;
    pos_str = hkv * dh;
    head_str = dh;
  }
  if (dh == 128)
    hipLaunchKernelGGL((decode_attn_kernel<128>), grid, dim3(256), 0, s,
                       (const short*)q, (const short*)kcache, (const short*)vcache,
                       block_table, seq_lens, (short*)o, (int)b, (int)h,
                       (int)hkv, (int)bs, (int)max_blocks, scale,
                       blk_str, pos_str, head_str);
  else
    hipLaunchKernelGGL((decode_attn_kernel<64>), grid, dim3(256), 0, s,
                       (const short*)q, (const short*)kcache, (const short*)vcache,
                       block_table, seq_lens, (short*)o, (int)b, (int)h,
                       (int)hkv, (int)bs, (int)max_blocks, scale,
                       blk_str, pos_str, head_str);
}

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

// int8 sibling of decode_attn_kernel: same decomposition (one 256-thread
// block per (b, q-head), online softmax, pipelined next-step loads, LDS slot
// merge by wave 0) with 16 codes = 16 B per lane in flight:
//   D/16 lanes per position (8 | 4), 64/(D/16) positions per wave step,
//   SLOTS = 4x that (32 | 64) merge slots, so[SLOTS][D] fp32 = 16 KB.
// Scales act on the result, not on the element: the softmax scale is folded
// into q, score = (sum q_i code_i) * d_k[pos], oacc += (p * d_v[pos]) * code.
// d_k / d_v load in the same prefetch stage as the codes.
template <int D>
__launch_bounds__(256)
__global__ void decode_attn_int8_kernel(
    const short* __restrict__ qg, const signed char* __restrict__ kcache,
    const signed char* __restrict__ vcache, const float* __restrict__ kscale,
    const float* __restrict__ vscale, const int* __restrict__ block_table,
    const int* __restrict__ seq_lens, short* __restrict__ og, int H, int HKV,
    int bs, int max_blocks, int nblocks, float scale, long long ss_blk,
    long long ss_pos, long long ss_head) {
  constexpr int LPP = D / 16;            // lanes per position
  constexpr int PPW = 64 / LPP;          // positions per wave step
  constexpr int SLOTS = 4 * PPW;         // positions per block step
  const int b = blockIdx.x / H;
  const int h = blockIdx.x % H;
  const int hkv = h / (H / HKV);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int lg = lane % LPP;             // 16-element group within D
  const int lp = lane / LPP;             // position slot within the wave
  // never walk past the table: entries beyond ceil(S/bs) are not read
  const int S = min(seq_lens[b], max_blocks * bs);

  float qv[16];
  {
    const short* qp = qg + ((long long)b * H + h) * D + lg * 16;
    const shortx8 q0 = *reinterpret_cast<const shortx8*>(qp);
    const shortx8 q1 = *reinterpret_cast<const shortx8*>(qp + 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      qv[i] = bf2f(q0[i]) * scale;
      qv[8 + i] = bf2f(q1[i]) * scale;
    }
  }

  float m = -1e30f, l = 0.f;  // finite sentinel: -ffast-math breaks +-inf
  float oacc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) oacc[i] = 0.f;

  auto load_kv = [&](int pos0, bool& ok, uint4& kw, uint4& vw, float& dk,
                     float& dv) {
    const int pos = pos0 + lp;
    ok = pos < S;
    if (ok) {
      const int phys = block_table[(long long)b * max_blocks + pos / bs];
      const int off = pos % bs;
      // a table entry outside the pool reads nothing (wrong numbers, no fault)
      ok = (unsigned)phys < (unsigned)nblocks;
      if (ok) {
        const long long row = ((long long)phys * bs + off) * HKV + hkv;
        const long long srow = (long long)phys * ss_blk +
                               (long long)off * ss_pos +
                               (long long)hkv * ss_head;
        kw = *reinterpret_cast<const uint4*>(kcache + row * D + lg * 16);
        vw = *reinterpret_cast<const uint4*>(vcache + row * D + lg * 16);
        dk = kscale[srow];
        dv = vscale[srow];
      }
    }
  };

  bool okc = false, okn = false;
  uint4 kc = make_uint4(0, 0, 0, 0), vc = kc, kn = kc, vn = kc;
  float dkc = 0.f, dvc = 0.f, dkn = 0.f, dvn = 0.f;
  const int p_start = wid * PPW;
  load_kv(p_start, okc, kc, vc, dkc, dvc);
  for (int pos0 = p_start; pos0 < S; pos0 += SLOTS) {
    if (pos0 + SLOTS < S) load_kv(pos0 + SLOTS, okn, kn, vn, dkn, dvn);
    else okn = false;
    const bool ok = okc;
    const unsigned kwd[4] = {kc.x, kc.y, kc.z, kc.w};
    const unsigned vwd[4] = {vc.x, vc.y, vc.z, vc.w};
    float sc = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) sc += qv[i] * code2f(kwd[i >> 2], i & 3);
    sc = group_reduce<LPP>(sc, SumOp());
    sc = ok ? sc * dkc : -1e30f;
    const float m_new = fmaxf(m, sc);
    const float corr = __expf(m - m_new);  // underflows to 0 for the sentinel
    const float p = ok ? __expf(sc - m_new) : 0.f;
    l = l * corr + p;
    m = m_new;
    const float pv = ok ? p * dvc : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      oacc[i] = oacc[i] * corr + pv * code2f(vwd[i >> 2], i & 3);
    okc = okn; kc = kn; vc = vn; dkc = dkn; dvc = dvn;
  }

  // ---- merge the SLOTS position-slot partials (4 waves x PPW slots) -------
  __shared__ float sm[SLOTS], sl[SLOTS];
  __shared__ __attribute__((aligned(16))) float so[SLOTS][D];
  const int slot_id = wid * PPW + lp;
  if (lg == 0) {
    sm[slot_id] = m;
    sl[slot_id] = l;
  }
#pragma unroll
  for (int i = 0; i < 16; i += 4) {
    floatx4 o4 = {oacc[i], oacc[i + 1], oacc[i + 2], oacc[i + 3]};
    *reinterpret_cast<floatx4*>(&so[slot_id][lg * 16 + i]) = o4;
  }
  __syncthreads();
  if (tid < 64) {
    // wave 0: lane owns D/64 output elements across all slots
    constexpr int EPL = D / 64;
    float gm = -1e30f;
#pragma unroll
    for (int s2 = 0; s2 < SLOTS; ++s2) gm = fmaxf(gm, sm[s2]);
    float gl = 0.f;
    float out[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) out[i] = 0.f;
#pragma unroll 8
    for (int s2 = 0; s2 < SLOTS; ++s2) {
      const float w = (sl[s2] > 0.f) ? __expf(sm[s2] - gm) : 0.f;
      gl += sl[s2] * w;
#pragma unroll
      for (int i = 0; i < EPL; ++i) out[i] += w * so[s2][lane * EPL + i];
    }
    const float inv = gl > 0.f ? 1.f / gl : 0.f;   // S == 0 -> zeros
    short* op = og + ((long long)b * H + h) * D + lane * EPL;
#pragma unroll
    for (int i = 0; i < EPL; ++i) op[i] = f2bf(out[i] * inv);
  }
}

void decode_attention_int8(const void* q, const void* kcache,
                           const void* vcache, const float* kscale,
                           const float* vscale, const int* block_table,
                           const int* seq_lens, void* o, int64_t b, int64_t h,
                           int64_t hkv, int64_t bs, int64_t max_blocks,
                           int64_t nblocks, int64_t dh, float scale,
                           int64_t ss_blk, int64_t ss_pos, int64_t ss_head,
                           hipStream_t s) {
  if (b * h == 0) return;
  dim3 grid((unsigned)(b * h));
#define PA_DA8_LAUNCH(DH)                                                     \
  hipLaunchKernelGGL((decode_attn_int8_kernel<DH>), grid, dim3(256), 0, s,    \
                     (const short*)q, (const signed char*)kcache,             \
                     (const signed char*)vcache, kscale, vscale, block_table, \
                     seq_lens, (short*)o, (int)h, (int)hkv, (int)bs,          \
                     (int)max_blocks, (int)nblocks, scale,                    \
                     (long long)ss_blk, (long long)ss_pos, (long long)ss_head)
  if (dh == 128) PA_DA8_LAUNCH(128);
  else PA_DA8_LAUNCH(64);
#undef PA_DA8_LAUNCH
}

}  // namespace pa
