// FlashAttention-2 forward for gfx950 (CDNA4): bf16, head_dim 64 / 128,
// causal or full, MHA / GQA, additive mask, Philox dropout, dense or varlen.
// Also the dropout keep-mask utility.  The backward is in fa_bwd.hip, the
// shared pieces in fa_common.h.
//
// Reference role: paddle/phi/kernels/gpu/flash_attn_kernel.cu:41 (thin
// dispatch into dynloaded libflashattn) -- here the FA2 algorithm is
// implemented natively for CDNA4 instead of vendoring a library.
//
// Design:
//   * mfma_f32_32x32x16_bf16; each wave owns 32 q rows; 4 waves/block
//     -> 128-row q blocks; KV tiles of 64.
//   * SWAPPED QK^T: S^T = mfma(K, Q) puts a full q-COLUMN of scores in
//     each lane (C layout col = lane&31 = q), so the online softmax is
//     per-lane scalar + ONE shfl_xor(32) -- no 16-lane reductions.
//   * P stays in registers: the PV A-fragments are assembled with packed
//     bf16 pairs + 2x permlane32_swap per k-step -- no P LDS round-trip,
//     no lgkmcnt(0) stall.
//   * K and V land once per tile, by async global_load_lds with a
//     pre-swizzled source column, in their natural [64 kv][D] image
//     (fa_common.h, fa_kv_off).  K feeds S^T by ds_read_b128 rows; V feeds
//     P V by ds_read_b64_tr_b16, so no transposed copy of V is built and
//     no VGPR-destination load is left in the loop of full tiles.  Two
//     {K, V} buffers, tile t+1 in flight under tile t's math, one barrier
//     per tile.  Every MFMA gets the operands, in the k order, of the
//     kernel this replaces (V^T by scalar writes), so O and LSE are
//     bit-identical to it.  Measured, B12 H32 S2048 D128 causal: 1366 ->
//     664 us per call in the flagship trace, SQ_LDS_BANK_CONFLICT 1.6e8 ->
//     0, 234 -> 210 VGPR (docs/KERNELS.md, "forward and dQ").
//   * defer-max rescale, boundary-only masking.
//   * LSE saved (fp32) for backward + ring/context-parallel merges.
#include "fa_common.h"

namespace pa {

// VARLEN: packed ragged batch (flash_attn_unpadded), see FaArgs / FaBlock.
template <int D, bool CAUSAL, bool MASKED, bool DROPOUT, bool VARLEN>
__launch_bounds__(256, 2)
__global__ void fa_fwd32_kernel(const FaArgs a) {
  const short* __restrict__ qg = (const short*)a.q;
  const short* __restrict__ kg = (const short*)a.k;
  const short* __restrict__ vg = (const short*)a.v;
  short* __restrict__ og = (short*)a.o;
  float* __restrict__ lseg = a.lse;
  const int H = a.h, Sq = a.sq, Skv = a.skv;
  const float scale = a.scale;
  const long long q_ss = a.q_s.s, k_ss = a.k_s.s, o_ss = a.o_s.s;
  const short* __restrict__ maskg = (const short*)a.mask;
  const long long m_sb = a.m_s.b, m_sh = a.m_s.h, m_sq = a.m_s.s;
  const float pdrop = a.pdrop;
  const unsigned long long rseed = a.seed, roffset = a.offset;
  constexpr int NW = 4;            // waves per block, 32 q rows each
  constexpr int NT = NW * 64;
  constexpr int QB = NW * 32;      // 128 q rows per block
  constexpr int KB = 64;           // kv tile
  constexpr int NKS = D / 16;      // q/k k-steps over head dim (mfma K=16)
  constexpr int NDT = D / 32;      // output d tiles (32 wide)
  constexpr int TILE = KB * D * 2;  // bytes of one [64][D] tile
  // one array (a second __shared__ object beside a DMA target can cost a
  // vmcnt(0) per LDS read): two {K, V} buffers, tile t+1 in flight while the
  // MFMAs chew tile t
  __shared__ __attribute__((aligned(16))) char lds[4 * TILE];

  // block index on the SLOW grid dim (y) so causal longest-first ordering
  // is global: the dispatcher walks x fastest, so a length-ordered y makes
  // the drain tail all-short blocks instead of one of each length.
  const FaBlock g = fa_block<VARLEN>(
      a, a.q_bmap, (CAUSAL ? (int)(gridDim.y - 1 - blockIdx.y) : (int)blockIdx.y) * QB);
  const int b = g.b, h = g.h, q0 = g.r0, Sq_e = g.Sq_e, Skv_e = g.Skv_e;
  const int cdelta = g.cdelta, qglob0 = g.q_tok0;
  const long long qbase = fa_base(g, a.q_s, h, g.q_tok0);
  const long long kbase = fa_base(g, a.k_s, h / (H / a.hkv), g.k_tok0);
  const long long obase = fa_base(g, a.o_s, h, g.q_tok0);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wq = tid >> 6;
  const int l32 = lane & 31;       // q column (C layout)
  const int hi = lane >> 5;        // half-wave id
  const int q0w = q0 + wq * 32;

  // Q fragments (B operand of the swapped QK^T): lane holds
  // Q[q0w + l32][16*ks + 8*hi .. +7].  Pre-scaled by softmax scale ONCE
  // here -- saves one VALU mul per score element in the kv loop (the
  // softmax block is what keeps this kernel VALU-issue-bound).
  shortx8 qf[NKS];
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
      } else {
        for (int i = 0; i < 8; ++i) qf[ks][i] = 0;
      }
    }
  }

  floatx16 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;   // stats for q column l32

  const int kv_end = CAUSAL ? min(Skv_e, q0 + QB + cdelta) : Skv_e;

  // LDS addresses of the lane's rows for the transposed reads of V
  const unsigned lds_a = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  unsigned tr_a[2][NDT];   // even, odd k-steps
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    tr_a[0][dt] = fa_tr_addr<D>(lds_a, lane, dt, 0);
    tr_a[1][dt] = fa_tr_addr<D>(lds_a, lane, dt, 16);
  }

  if (kv_end > 0) fa_stage_kv<D, NT>(lds, kg, vg, kbase, k_ss, 0, Skv_e, tid);
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
    if (kv0 + KB < kv_end)
      fa_stage_kv<D, NT>(lds + (cur ^ 1) * (2 * TILE), kg, vg, kbase, k_ss, kv0 + KB, Skv_e, tid);
    cur ^= 1;

    // ---- S^T = K Q^T : 2 kv tiles of 32 -----------------------------------
    floatx16 st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[t][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        shortx8 kf = *reinterpret_cast<const shortx8*>(
            k_t + fa_kv_off<D>(t * 32 + l32, ks * 2 + hi));
        st[t] = mfma32_bf16(kf, qf[ks], st[t]);
      }
    }

    // ---- mask + scale + per-lane online softmax ---------------------------
    const int q_abs = q0w + l32;
    if (MASKED && q_abs < Sq_e) {
      // additive mask [B, 1|H, Sq, Skv]; reg groups are 4 consecutive kv
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
    float mx = -INFINITY;
    const bool boundary = (kv0 + KB > Skv_e) || (CAUSAL && kv0 + KB > q_abs + cdelta);
    if (boundary) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int kv_abs = kv0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hi;
          float v = st[t][r];                 // Q pre-scaled at load
          if (kv_abs >= Skv_e || (CAUSAL && kv_abs > q_abs + cdelta)) v = -INFINITY;
          st[t][r] = v;
          mx = fmaxf(mx, v);
        }
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          mx = fmaxf(mx, st[t][r]);           // Q pre-scaled at load
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float THR = 8.f;
    // per-lane stats are divergent; compute corr for every lane so the
    // broadcast shfl below is wave-uniform-safe, and vote before paying
    // for the O rescale
    const bool grow = (mx > m_run + THR) || (m_run == -INFINITY);
    float m_new = grow ? fmaxf(m_run, mx) : m_run;
    float corr = (m_run == -INFINITY) ? 0.f : __expf(m_run - m_new);
    if (__any(grow && m_run != -INFINITY)) {
      l_run *= corr;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int rq = (r & 3) + 8 * (r >> 2) + 4 * hi;
          float c = __shfl(corr, rq, 64);
          oacc[dt][r] *= c;
        }
    }
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p = (st[t][r] == -INFINITY) ? 0.f : __expf(st[t][r] - m_run);
        st[t][r] = p;
        psum += p;
      }
    psum += __shfl_xor(psum, 32, 64);
    l_run += psum;
    if (DROPOUT) {
      // Philox keep-mask on P (normalizer above uses undropped P)
      const float inv_keep = 1.f / (1.f - pdrop);
      const unsigned thr24 = (unsigned)(pdrop * 16777216.f);
      const long long bh_ll = (long long)b * H + h;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          long long kvb = kv0 + 32 * t + 8 * g + 4 * hi;
          long long elem = (bh_ll * Sq + (q_abs + qglob0)) * (long long)Skv + kvb;
          uintx4 rv = philox10(rseed, roffset + (unsigned long long)(elem >> 2));
#pragma unroll
          for (int j = 0; j < 4; ++j)
            st[t][4 * g + j] = ((rv[j] >> 8) >= thr24)
                                   ? st[t][4 * g + j] * inv_keep : 0.f;
        }
    }

    // ---- O += P V : assemble P A-frags in-register ------------------------
    // one k-step of 16 kv rows; KS is a type so the offsets of the
    // transposed reads are immediates
    auto pv_step = [&](auto KS) {
      constexpr int ks = decltype(KS)::value;
      constexpr int t = ks >> 1;
      constexpr int kp = ks & 1;
      // STATIC register indices only (rule #20: a runtime `hi` index into
      // the v16 accumulator becomes a 16-way cndmask tree); pack all four
      // candidate words, then one select each by hi.
      const int b0 = 8 * kp;
      int P0 = pack_bf2(st[t][b0 + 0], st[t][b0 + 1]);
      int P1 = pack_bf2(st[t][b0 + 2], st[t][b0 + 3]);
      int P2 = pack_bf2(st[t][b0 + 4], st[t][b0 + 5]);
      int P3 = pack_bf2(st[t][b0 + 6], st[t][b0 + 7]);
      int O1 = hi ? P2 : P0;             // own reg-group words
      int O2 = hi ? P3 : P1;
      int S1 = hi ? P0 : P2;             // supply (partner's) words
      int S2 = hi ? P1 : P3;
      intx2 ra = __builtin_amdgcn_permlane32_swap(S1, S2, false, false);
      intx2 rb = __builtin_amdgcn_permlane32_swap(S2, S1, false, false);
      // lanes<32: partner supply = (ra[1], rb[1]); lanes>=32: (rb[0], ra[0])
      int X1 = hi ? rb[0] : ra[1];
      int X2 = hi ? ra[0] : rb[1];
      // A-frag words in kv order: hi==0 -> {own, partner}; hi==1 -> {partner, own}
      intx4 paw;
      paw[0] = hi ? X1 : O1;
      paw[1] = hi ? X2 : O2;
      paw[2] = hi ? O1 : X1;
      paw[3] = hi ? O2 : X2;
      shortx8 pa = *reinterpret_cast<shortx8*>(&paw);
      // B[k = 16*ks + 8*hi + 0..7][n = 32*dt + l32] of V, by transposed reads
      shortx8 vf[NDT];
      unsigned va[NDT];
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) va[dt] = boff + tr_a[kp][dt];
      fa_tr_read<D, TILE + ks * 16 * D * 2>(vf, va);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) oacc[dt] = mfma32_bf16(pa, vf[dt], oacc[dt]);
    };
    pv_step(std::integral_constant<int, 0>{});
    pv_step(std::integral_constant<int, 1>{});
    pv_step(std::integral_constant<int, 2>{});
    pv_step(std::integral_constant<int, 3>{});
  }

  // ---- epilogue: O /= l, store O + LSE ------------------------------------
  float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int rq = (r & 3) + 8 * (r >> 2) + 4 * hi;
    float il = __shfl(inv_l, rq, 64);
    int row = q0w + rq;
    if (row >= Sq_e) continue;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      og[obase + (long long)row * o_ss + dt * 32 + l32] = f2bf(oacc[dt][r] * il);
  }
  if (hi == 0 && q0w + l32 < Sq_e)
    lseg[(long long)(b * H + h) * Sq + qglob0 + q0w + l32] =
        (l_run > 0.f) ? m_run + __logf(l_run) : -INFINITY;
}

void flash_attn_fwd(const FaArgs& a, hipStream_t s) {
  const bool varlen = a.cu_q != nullptr;
  const dim3 grid((unsigned)(a.b * a.h),
                  (unsigned)(varlen ? a.n_qblocks : cdiv(a.sq, 128)));
  fa_dispatch(a, [&](auto D, auto C, auto M, auto P) {
    if (!varlen)
      hipLaunchKernelGGL((fa_fwd32_kernel<D(), C(), M(), P(), false>), grid, dim3(256), 0, s, a);
    else if constexpr (!M())   // varlen takes no mask
      hipLaunchKernelGGL((fa_fwd32_kernel<D(), C(), false, P(), true>), grid, dim3(256), 0, s, a);
  });
}

// debug/test utility: materialize the attention-dropout keep mask the FA
// kernels derive from (seed, offset) -- lets tests compare fwd/bwd against
// an exact CPU oracle using the same mask.
__global__ void fa_dropout_mask_kernel(unsigned char* __restrict__ out,
                                       float p, unsigned long long seed,
                                       unsigned long long offset,
                                       long long total) {
  long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long base = i4 * 4;
  if (base >= total) return;
  unsigned thr24 = (unsigned)(p * 16777216.f);
  uintx4 rv = philox10(seed, offset + (unsigned long long)i4);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (base + j < total) out[base + j] = ((rv[j] >> 8) >= thr24) ? 1 : 0;
}

void fa_dropout_mask(void* out, int64_t total, float p, uint64_t seed,
                     uint64_t offset, hipStream_t s) {
  long long n4 = (total + 3) / 4;
  dim3 g((unsigned)hmin<long long>((n4 + 255) / 256, 1 << 30));
  hipLaunchKernelGGL(fa_dropout_mask_kernel, g, dim3(256), 0, s,
                     (unsigned char*)out, p, seed, offset, total);
}

}  // namespace pa
