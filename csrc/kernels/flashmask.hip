// FlashMask attention for gfx950 (CDNA4): flash attention under a column-
// sparse mask.  For key column j, startend_row_indices names up to two
// half-open ranges of query rows that may not see j,
//     M_j = [lo0, hi0) u [lo1, hi1),
// on top of the optional top-left causal mask.  A score is untouched or
// removed; a row with no visible column gives O = 0, LSE = -inf, dQ = 0 and
// adds nothing to dK / dV.  bf16, head_dim 64 / 128, dense, no dropout.
//
// Kernels (all over the fa_common.h helpers; fa_fwd32.hip and fa_bwd.hip hold
// the kernels these are derived from and are not touched: this file is built
// without packed-fp32 VALU ops, which a flavour inside those files could not
// be without moving their instantiations):
//   * flashmask_prep_kernel: one launch, any of the four (causal, C) forms ->
//       bounds int32 [B, Hm, 4, Skv8]  lo0 | hi0 | lo1 | hi1, bound-major,
//              Skv8 = Skv rounded up to 8, pad columns empty (Sq, Sq);
//       tiles  int32 [B, Hm, ceil(Skv/64), 8] per 64-column tile and range i
//              {max lo_i, min hi_i, min lo_i, max hi_i} over the tile's real
//              columns.  A wave per tile, shuffles only: no atomics, no host
//              read, every element written, graph-capturable.
//   * flashmask_fwd_kernel / flashmask_dq_kernel: the 128-row q block, 64-column
//     kv tile, two {K, V} DMA buffers and one barrier per tile of the dense
//     kernels, but the walk is kv0 = next_live(kv0 + 64): a tile is dead for
//     the block when some range has q0 >= max lo and min(q0+128, Sq) <= min
//     hi.  Dead tiles are never staged; buffer parity counts live tiles.  The
//     next tile is tested with uniform loads; a run of dead tiles is crossed
//     64 summaries at a time (one per lane, a ballot), so a leading run of
//     hundreds of tiles costs a handful of loads.  Per live tile each wave
//     classifies its own 32 rows from the summary: all masked -> no MFMAs
//     (barrier and staging still taken); outside [min lo, max hi) of every
//     live range -> the dense path, no bound loads; else 16-byte bound loads
//     per 4-column register group and a predicate.
//   * flashmask_dkv_kernel: dK or dV (one launch each), a 128-column kv block,
//     a lane per column, 32-row q tiles.  The lane keeps its column's bounds
//     in registers; the block takes max lo / min hi of its columns from the
//     tile summary and the q stream jumps every run of fully masked q tiles
//     before the next tile is staged, so the double buffer never holds a
//     skipped tile.
// P and dS are zeroed by predicate; nothing relies on arithmetic with
// lse = -inf (-ffast-math): the backward reads lse = -inf as +1e30.
#include "fa_common.h"

namespace pa {

// ---------------------------------------------------------------------------
// prep
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void flashmask_prep_kernel(
    const int* __restrict__ idx, int* __restrict__ bounds, int* __restrict__ tiles,
    int Sq, int Skv, int Skv8, int C, int causal) {
  const int t = blockIdx.x, lane = threadIdx.x;
  const long long bh = blockIdx.y;          // batch * Hm + mask head
  const int j = t * 64 + lane;
  const bool real = j < Skv;
  int lo0 = Sq, hi0 = Sq, lo1 = Sq, hi1 = Sq;
  if (real) {
    const int* p = idx + (bh * Skv + j) * C;
    lo0 = p[0];
    if (causal) {
      if (C == 2) hi0 = p[1];
    } else if (C == 2) {
      lo1 = 0; hi1 = p[1];
    } else {
      hi0 = p[1]; lo1 = p[2]; hi1 = p[3];
    }
    lo0 = min(max(lo0, 0), Sq); hi0 = min(max(hi0, 0), Sq);
    lo1 = min(max(lo1, 0), Sq); hi1 = min(max(hi1, 0), Sq);
    if (lo0 >= hi0) { lo0 = Sq; hi0 = Sq; }
    if (lo1 >= hi1) { lo1 = Sq; hi1 = Sq; }
  }
  if (j < Skv8) {
    int* bp = bounds + bh * 4 * Skv8 + j;
    bp[0] = lo0; bp[Skv8] = hi0; bp[2 * (long long)Skv8] = lo1; bp[3 * (long long)Skv8] = hi1;
  }
  // bounds lie in [0, Sq]: 0 / Sq are neutral for max / min over real columns
  int r[8] = {real ? lo0 : 0, real ? hi0 : Sq, real ? lo0 : Sq, real ? hi0 : 0,
              real ? lo1 : 0, real ? hi1 : Sq, real ? lo1 : Sq, real ? hi1 : 0};
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int o = __shfl_xor(r[i], off, 64);
      r[i] = ((i & 3) == 0 || (i & 3) == 3) ? max(r[i], o) : min(r[i], o);
    }
  if (lane == 0) {
    intx4* tp = reinterpret_cast<intx4*>(tiles + (bh * gridDim.x + t) * 8);
    tp[0] = intx4{r[0], r[1], r[2], r[3]};
    tp[1] = intx4{r[4], r[5], r[6], r[7]};
  }
}

void flashmask_prep(const int* idx, int* bounds, int* tiles, int64_t b_hm, int64_t sq,
                    int64_t skv, int c, bool causal, hipStream_t s) {
  const dim3 grid((unsigned)cdiv(skv, 64), (unsigned)b_hm);
  hipLaunchKernelGGL(flashmask_prep_kernel, grid, dim3(64), 0, s, idx, bounds, tiles,
                     (int)sq, (int)skv, (int)((skv + 7) / 8 * 8), c, (int)causal);
}

// ---------------------------------------------------------------------------
// the tile walk of the forward and of dQ
// ---------------------------------------------------------------------------
// rows [r0, r1) all lie in range i of every column of the summarised tile
__device__ __forceinline__ bool fm_all_masked(const int* s, int r0, int r1, int nr) {
  bool d = r0 >= s[0] && r1 <= s[1];
  if (nr > 1) d = d || (r0 >= s[4] && r1 <= s[5]);
  return d;
}

// rows [r0, r1) touch range i of some column of the summarised tile
__device__ __forceinline__ bool fm_touched(const int* s, int r0, int r1, int nr) {
  bool p = r1 > s[2] && r0 < s[3];
  if (nr > 1) p = p || (r1 > s[6] && r0 < s[7]);
  return p;
}

// first kv0' >= kv0 (a multiple of 64) below kv_end whose tile is live for
// rows [q0, qe), or a value >= kv_end.  Block-uniform: every argument but
// `lane` is, and the result of the ballot is.
__device__ __forceinline__ int fm_next_live(const int* __restrict__ ts, int kv0, int kv_end,
                                            int q0, int qe, int nr, int lane) {
  if (kv0 >= kv_end) return kv0;
  int t = kv0 >> 6;
  if (!fm_all_masked(ts + t * 8, q0, qe, nr)) return kv0;
  const int t_end = (kv_end + 63) >> 6;
  for (t += 1; t < t_end; t += 64) {
    const int tt = t + lane;
    bool live = false;
    if (tt < t_end) {
      const intx2 a = *reinterpret_cast<const intx2*>(ts + tt * 8);
      bool d = q0 >= a[0] && qe <= a[1];
      if (nr > 1) {
        const intx2 c = *reinterpret_cast<const intx2*>(ts + tt * 8 + 4);
        d = d || (q0 >= c[0] && qe <= c[1]);
      }
      live = !d;
    }
    const unsigned long long m = __ballot(live);
    if (m) return (t + __ffsll((long long)m) - 1) << 6;
  }
  return t_end << 6;
}

// what a block needs of the mask: its head's bounds and tile summaries
struct FmView {
  const int* __restrict__ bnd;   // [4][Skv8]
  const int* __restrict__ ts;    // [ceil(Skv/64)][8]
  int Skv8, nr;
};

__device__ __forceinline__ FmView fm_view(const FaArgs& a, int b, int kvhead) {
  const int Skv8 = (a.skv + 7) & ~7, ntl = (a.skv + 63) >> 6;
  const long long mh = (long long)b * a.fm_hm + (a.fm_hm > 1 ? kvhead : 0);
  return {a.fm_bounds + mh * 4 * Skv8, a.fm_tiles + mh * ntl * 8, Skv8, a.fm_nr};
}

// lane's row `q` against the bounds of columns kvb..kvb+3 (kvb a multiple of
// 4): bit j set = masked.  Columns past Skv8 report nothing: the tail
// predicate owns them.
__device__ __forceinline__ unsigned fm_group_mask(const FmView& m, int kvb, int q) {
  unsigned r = 0;
  if (kvb < m.Skv8) {
    const intx4 lo = *reinterpret_cast<const intx4*>(m.bnd + kvb);
    const intx4 hi = *reinterpret_cast<const intx4*>(m.bnd + m.Skv8 + kvb);
#pragma unroll
    for (int j = 0; j < 4; ++j) r |= (unsigned)(q >= lo[j] && q < hi[j]) << j;
    if (m.nr > 1) {
      const intx4 lo1 = *reinterpret_cast<const intx4*>(m.bnd + 2 * m.Skv8 + kvb);
      const intx4 hi1 = *reinterpret_cast<const intx4*>(m.bnd + 3 * m.Skv8 + kvb);
#pragma unroll
      for (int j = 0; j < 4; ++j) r |= (unsigned)(q >= lo1[j] && q < hi1[j]) << j;
    }
  }
  return r;
}

// the lane's row `q` against the 64 columns of the tile at kv0: bit 16*t + r =
// score register st[t][r] is masked.  Taken before the MFMAs of the tile, so
// the bound loads never hold registers beside the S / dP accumulators.
__device__ __forceinline__ unsigned fm_tile_mask(const FmView& m, int kv0, int hi, int q) {
  unsigned bits = 0;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int gr = 0; gr < 4; ++gr)
      bits |= fm_group_mask(m, kv0 + 32 * t + 8 * gr + 4 * hi, q) << (16 * t + 4 * gr);
  return bits;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int D, bool CAUSAL>
__launch_bounds__(256, 2)
__global__ void flashmask_fwd_kernel(const FaArgs a) {
  const short* __restrict__ qg = (const short*)a.q;
  const short* __restrict__ kg = (const short*)a.k;
  const short* __restrict__ vg = (const short*)a.v;
  short* __restrict__ og = (short*)a.o;
  float* __restrict__ lseg = a.lse;
  const int H = a.h, Sq = a.sq, Skv = a.skv;
  const float scale = a.scale;
  const long long q_ss = a.q_s.s, k_ss = a.k_s.s, o_ss = a.o_s.s;
  constexpr int NW = 4;
  constexpr int NT = NW * 64;
  constexpr int QB = NW * 32;
  constexpr int KB = 64;
  constexpr int NKS = D / 16;
  constexpr int NDT = D / 32;
  constexpr int TILE = KB * D * 2;
  __shared__ __attribute__((aligned(16))) char lds[4 * TILE];

  const FaBlock g = fa_block<false>(
      a, nullptr, (CAUSAL ? (int)(gridDim.y - 1 - blockIdx.y) : (int)blockIdx.y) * QB);
  const int b = g.b, h = g.h, q0 = g.r0;
  const int kvhead = h / (H / a.hkv);
  const long long qbase = fa_base(g, a.q_s, h, 0);
  const long long kbase = fa_base(g, a.k_s, kvhead, 0);
  const long long obase = fa_base(g, a.o_s, h, 0);
  const FmView fm = fm_view(a, b, kvhead);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31;
  const int hi = lane >> 5;
  const int q0w = q0 + wq * 32;
  const int qe = min(q0 + QB, Sq), qew = min(q0w + 32, Sq);

  // Q fragments, pre-scaled once (fa_fwd32_kernel)
  shortx8 qf[NKS];
  {
    int row = q0w + l32;
    bool ok = row < Sq;
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
  // Removed scores and the empty running maximum are FM_NEG, a finite
  // sentinel told apart by an ordered compare: with -ffast-math a compare
  // against -inf may be folded away, and exp(-inf - -inf) is NaN for a row
  // whose columns so far are all masked.
  constexpr float FM_NEG = -1e30f, FM_CUT = -1e29f;
  float m_run = FM_NEG, l_run = 0.f;

  const int kv_end = CAUSAL ? min(Skv, q0 + QB) : Skv;

  const unsigned lds_a = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  unsigned tr_a[2][NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    tr_a[0][dt] = fa_tr_addr<D>(lds_a, lane, dt, 0);
    tr_a[1][dt] = fa_tr_addr<D>(lds_a, lane, dt, 16);
  }

  int kv0 = fm_next_live(fm.ts, 0, kv_end, q0, qe, fm.nr, lane);
  if (kv0 < kv_end) fa_stage_kv<D, NT>(lds, kg, vg, kbase, k_ss, kv0, Skv, tid);
  int cur = 0;   // parity over live tiles
  while (kv0 < kv_end) {
    // as fa_fwd32_kernel: the tile was issued one live tile ago and nothing
    // newer is in flight; the barrier also frees the other buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned boff = cur * (2 * TILE);
    const char* k_t = lds + boff;
    const int kvn = fm_next_live(fm.ts, kv0 + KB, kv_end, q0, qe, fm.nr, lane);
    if (kvn < kv_end)
      fa_stage_kv<D, NT>(lds + (cur ^ 1) * (2 * TILE), kg, vg, kbase, k_ss, kvn, Skv, tid);
    cur ^= 1;

    const int* sum = fm.ts + (kv0 >> 6) * 8;
    // a wave whose rows are all masked in this tile (or past Sq) has p = 0
    // throughout: its running stats and O do not move
    if (q0w < Sq && !fm_all_masked(sum, q0w, qew, fm.nr)) {
      const int q_abs = q0w + l32;
      const bool touched = fm_touched(sum, q0w, qew, fm.nr);
      unsigned mbits = 0;
      if (touched) mbits = fm_tile_mask(fm, kv0, hi, q_abs);
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

      if (touched) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (mbits & (1u << (16 * t + r))) st[t][r] = FM_NEG;
      }
      float mx = FM_NEG;
      const bool boundary = (kv0 + KB > Skv) || (CAUSAL && kv0 + KB > q_abs);
      if (boundary) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            int kv_abs = kv0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hi;
            float v = st[t][r];
            if (kv_abs >= Skv || (CAUSAL && kv_abs > q_abs)) v = FM_NEG;
            st[t][r] = v;
            mx = fmaxf(mx, v);
          }
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[t][r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float THR = 8.f;
      const bool first = m_run < FM_CUT;
      const bool grow = (mx > m_run + THR) || first;
      float m_new = grow ? fmaxf(m_run, mx) : m_run;
      float corr = first ? 0.f : __expf(m_run - m_new);
      if (__any(grow && !first)) {
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
          float p = (st[t][r] < FM_CUT) ? 0.f : __expf(st[t][r] - m_run);
          st[t][r] = p;
          psum += p;
        }
      psum += __shfl_xor(psum, 32, 64);
      l_run += psum;

      // O += P V (fa_fwd32_kernel's in-register A fragments)
      auto pv_step = [&](auto KS) {
        constexpr int ks = decltype(KS)::value;
        constexpr int t = ks >> 1;
        constexpr int kp = ks & 1;
        const int b0 = 8 * kp;
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
    kv0 = kvn;
  }

  // a block or a row with no live column: l_run = 0 -> O = 0, LSE = -inf
  float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int rq = (r & 3) + 8 * (r >> 2) + 4 * hi;
    float il = __shfl(inv_l, rq, 64);
    int row = q0w + rq;
    if (row >= Sq) continue;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      og[obase + (long long)row * o_ss + dt * 32 + l32] = f2bf(oacc[dt][r] * il);
  }
  if (hi == 0 && q0w + l32 < Sq)
    lseg[(long long)(b * H + h) * Sq + q0w + l32] =
        (l_run > 0.f) ? m_run + __logf(l_run) : __int_as_float(0xff800000);   // -inf
}

// ---------------------------------------------------------------------------
// dQ
// ---------------------------------------------------------------------------
template <int D, bool CAUSAL>
__launch_bounds__(256, 2)
__global__ void flashmask_dq_kernel(const FaArgs a) {
  const short* __restrict__ dog = (const short*)a.dout;
  const short* __restrict__ qg = (const short*)a.q;
  const short* __restrict__ kg = (const short*)a.k;
  const short* __restrict__ vg = (const short*)a.v;
  const float* __restrict__ lseg = a.lse;
  const float* __restrict__ deltag = a.delta;
  short* __restrict__ dqg = (short*)a.dq;
  const int H = a.h, Sq = a.sq, Skv = a.skv;
  const float scale = a.scale;
  const long long q_ss = a.q_s.s, k_ss = a.k_s.s, do_ss = a.do_s.s, dq_ss = a.dq_s.s;
  constexpr int NW = 4;
  constexpr int NT = NW * 64;
  constexpr int QB = NW * 32;
  constexpr int KB = 64;
  constexpr int NKS = D / 16;
  constexpr int NDT = D / 32;
  constexpr int TILE = KB * D * 2;
  __shared__ __attribute__((aligned(16))) char lds[4 * TILE];

  const FaBlock g = fa_block<false>(
      a, nullptr, (CAUSAL ? (int)(gridDim.y - 1 - blockIdx.y) : (int)blockIdx.y) * QB);
  const int b = g.b, h = g.h, q0 = g.r0;
  const int kvhead = h / (H / a.hkv);
  const long long qbase = fa_base(g, a.q_s, h, 0);
  const long long dobase = fa_base(g, a.do_s, h, 0);
  const long long dqbase = fa_base(g, a.dq_s, h, 0);
  const long long kvbase = fa_base(g, a.k_s, kvhead, 0);
  const long long lse_base = (long long)(b * H + h) * Sq;
  const FmView fm = fm_view(a, b, kvhead);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31;
  const int hi = lane >> 5;
  const int q0w = q0 + wq * 32;
  const int qe = min(q0 + QB, Sq), qew = min(q0w + 32, Sq);

  shortx8 qf[NKS], dof[NKS];
  {
    int row = q0w + l32;
    bool ok = row < Sq;
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
  // a row past Sq or with no visible column (lse = -inf): exp(s - 1e30) = 0
  float lse_v = 1e30f, delta_v = 0.f;
  if (q_abs < Sq) {
    const float l = lseg[lse_base + q_abs];
    if (l > -1e30f) lse_v = l;
    delta_v = deltag[lse_base + q_abs];
  }

  floatx16 dq_acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;

  const unsigned lds_a = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  unsigned tr_a[2][NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    tr_a[0][dt] = fa_tr_addr<D>(lds_a, lane, dt, 0);
    tr_a[1][dt] = fa_tr_addr<D>(lds_a, lane, dt, 16);
  }

  const int kv_end = CAUSAL ? min(Skv, q0 + QB) : Skv;
  int kv0 = fm_next_live(fm.ts, 0, kv_end, q0, qe, fm.nr, lane);
  if (kv0 < kv_end) fa_stage_kv<D, NT>(lds, kg, vg, kvbase, k_ss, kv0, Skv, tid);
  int cur = 0;   // parity over live tiles
  while (kv0 < kv_end) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned boff = cur * (2 * TILE);
    const char* k_t = lds + boff;
    const char* v_t = k_t + TILE;
    const int kvn = fm_next_live(fm.ts, kv0 + KB, kv_end, q0, qe, fm.nr, lane);
    if (kvn < kv_end)
      fa_stage_kv<D, NT>(lds + (cur ^ 1) * (2 * TILE), kg, vg, kvbase, k_ss, kvn, Skv, tid);
    cur ^= 1;

    const int* sum = fm.ts + (kv0 >> 6) * 8;
    if (q0w < Sq && !fm_all_masked(sum, q0w, qew, fm.nr)) {
      const bool touched = fm_touched(sum, q0w, qew, fm.nr);
      unsigned mbits = 0;
      if (touched) mbits = fm_tile_mask(fm, kv0, hi, q_abs);
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

      // dS^T = P^T (dP^T - delta) * scale, P zeroed by predicate
      const bool bnd = (kv0 + KB > Skv) || (CAUSAL && kv0 + KB > q_abs);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float p = __expf(st[t][r] - lse_v);
          if (bnd) {
            int kv_abs = kv0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (kv_abs >= Skv || (CAUSAL && kv_abs > q_abs)) p = 0.f;
          }
          if (touched && (mbits & (1u << (16 * t + r)))) p = 0.f;
          st[t][r] = p * (dp[t][r] - delta_v) * scale;
        }

      // dQ += dS K (fa_bwd_dq32_kernel's in-register A fragments)
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
    kv0 = kvn;
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int rq = (r & 3) + 8 * (r >> 2) + 4 * hi;
    int row = q0w + rq;
    if (row >= Sq) continue;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      dqg[dqbase + (long long)row * dq_ss + dt * 32 + l32] = f2bf(dq_acc[dt][r]);
  }
}

// ---------------------------------------------------------------------------
// dK / dV: fa_bwd_dkv32_kernel's orientation (P = mfma(Q, K), the kv column in
// the lane, P / dS as B fragments by pack + permlane32_swap, the transposed
// operand dO^T or Q^T staged in LDS, two buffers), hkv == h.
// ---------------------------------------------------------------------------
template <int D, bool CAUSAL, bool IS_DK>
__launch_bounds__(256, 2)
__global__ void flashmask_dkv_kernel(const FaArgs a) {
  const short* __restrict__ dog = (const short*)a.dout;
  const short* __restrict__ qg = (const short*)a.q;
  const short* __restrict__ kg = (const short*)a.k;
  const short* __restrict__ vg = (const short*)a.v;
  const float* __restrict__ lseg = a.lse;
  const float* __restrict__ deltag = a.delta;
  short* __restrict__ outg = (short*)(IS_DK ? a.dk : a.dv);
  const int H = a.h, Sq = a.sq, Skv = a.skv;
  const float scale = a.scale;
  const long long q_ss = a.q_s.s, k_ss = a.k_s.s, do_ss = a.do_s.s, dk_ss = a.dk_s.s;
  constexpr int NW = 4;
  constexpr int NT = NW * 64;
  constexpr int KVB = NW * 32;
  constexpr int QT = 32;
  constexpr int NKS = D / 16;
  constexpr int NDT = D / 32;
  constexpr unsigned TR_RS = 64 * 2;
  __shared__ char t_lds[2][D * 64 * 2];
  __shared__ float stat_s[2][2 * QT];  // [lse | delta]

  const int kvblk = blockIdx.y;
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int kv0 = kvblk * KVB;
  const long long qbase = (long long)b * a.q_s.b + (long long)h * a.q_s.h;
  const long long dobase = (long long)b * a.do_s.b + (long long)h * a.do_s.h;
  const long long kvbase = (long long)b * a.k_s.b + (long long)h * a.k_s.h;
  const long long outbase = (long long)b * a.dk_s.b + (long long)h * a.dk_s.h;
  const long long lse_base = (long long)bh * Sq;
  const FmView fm = fm_view(a, b, h);
  const int nr = fm.nr;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wq = tid >> 6;
  const int l32 = lane & 31;
  const int hi = lane >> 5;
  const int kv0w = kv0 + wq * 32;
  const int kv_lane = kv0w + l32;

  shortx8 kf[NKS], vf[IS_DK ? NKS : 1];
  // the lane's column: canonical bounds, empty past Skv
  int lo0 = Sq, hi0 = Sq, lo1 = Sq, hi1 = Sq;
  {
    bool ok = kv_lane < Skv;
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
    if (ok) {
      lo0 = fm.bnd[kv_lane];
      hi0 = fm.bnd[fm.Skv8 + kv_lane];
      if (nr > 1) {
        lo1 = fm.bnd[2 * fm.Skv8 + kv_lane];
        hi1 = fm.bnd[3 * fm.Skv8 + kv_lane];
      }
    }
  }

  // the block's columns, from the summaries of its one or two 64-column
  // tiles: [ja, jb) = q tiles masked for every column, per range, in whole
  // q tiles (a range that reaches Sq takes the tail tile with it);
  // [mlo, mhi) = rows some column masks
  int ja[2], jb[2], mlo[2], mhi[2];
  {
    const int ntl = (Skv + 63) >> 6;
    const int* s0 = fm.ts + (2 * kvblk) * 8;
    const int* s1 = fm.ts + min(2 * kvblk + 1, ntl - 1) * 8;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int maxlo = max(s0[4 * i], s1[4 * i]), minhi = min(s0[4 * i + 1], s1[4 * i + 1]);
      ja[i] = (maxlo + QT - 1) & ~(QT - 1);
      jb[i] = minhi >= Sq ? (Sq + QT - 1) & ~(QT - 1) : minhi & ~(QT - 1);
      mlo[i] = min(s0[4 * i + 2], s1[4 * i + 2]);
      mhi[i] = max(s0[4 * i + 3], s1[4 * i + 3]);
    }
    if (nr < 2) { ja[1] = jb[1] = 0; mlo[1] = mhi[1] = 0; }
  }
  // ranges may abut (rows [0, 64) by one, [64, 200) by the other)
  auto jump = [&](int qn) {
    if (qn >= ja[1] && qn < jb[1]) qn = jb[1];
    if (qn >= ja[0] && qn < jb[0]) qn = jb[0];
    if (qn >= ja[1] && qn < jb[1]) qn = jb[1];
    return qn;
  };

  floatx16 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;

  auto stage = [&](int buf, int q0) {
    if (tid < QT) {
      int qa = q0 + tid;
      float l = 1e30f;
      if (qa < Sq) {
        const float lv = lseg[lse_base + qa];
        if (lv > -1e30f) l = lv;    // lse = -inf: a row with no visible column
      }
      stat_s[buf][tid] = l;
      if (IS_DK)
        stat_s[buf][QT + tid] = (qa < Sq) ? deltag[lse_base + qa] : 0.f;
    }
    const int rot = tid & 7;
    for (int flat = tid * 8; flat < QT * D; flat += NT * 8) {
      int row = flat / D, col = flat % D;
      shortx8 v;
      if (q0 + row < Sq) {
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

  const int q_start = jump(CAUSAL ? (kv0 / QT) * QT : 0);
  if (q_start < Sq) stage(0, q_start);
  __syncthreads();
  int cur = 0;
  for (int q0 = q_start, qn; q0 < Sq; q0 = qn) {
    qn = jump(q0 + QT);
    if (qn < Sq) stage(cur ^ 1, qn);

    const int q_lane = q0 + l32;
    const bool qok = q_lane < Sq;
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

    const bool bnd = (q0 + QT > Sq) || (kv0w + 32 > Skv) || (CAUSAL && kv0w + 32 > q0);
    const bool fmq = (q0 + QT > mlo[0] && q0 < mhi[0]) || (q0 + QT > mlo[1] && q0 < mhi[1]);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rq = (r & 3) + 8 * (r >> 2) + 4 * hi;
      const int q_abs = q0 + rq;
      float p = __expf(st[r] * scale - stat_s[cur][rq]);
      if (bnd) {
        if (q_abs >= Sq || kv_lane >= Skv || (CAUSAL && kv_lane > q_abs)) p = 0.f;
      }
      if (fmq) {
        if ((q_abs >= lo0 && q_abs < hi0) || (q_abs >= lo1 && q_abs < hi1)) p = 0.f;
      }
      st[r] = IS_DK ? p * (dp[r] - stat_s[cur][QT + rq]) * scale : p;
    }

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
  }

  if (kv_lane < Skv) {
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
// launchers: flash_attn_fwd / flash_attn_bwd (after delta) hand over here
// when FaArgs carries FlashMask tensors
// ---------------------------------------------------------------------------
template <class F>
static inline void fm_dispatch(const FaArgs& a, F&& f) {
  fa_bool(a.dh == 128, [&](auto d128) {
    fa_bool(a.causal, [&](auto c) {
      f(std::integral_constant<int, decltype(d128)::value ? 128 : 64>{}, c);
    });
  });
}

void flashmask_attn_fwd(const FaArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)(a.b * a.h), (unsigned)cdiv(a.sq, 128));
  fm_dispatch(a, [&](auto D, auto C) {
    hipLaunchKernelGGL((flashmask_fwd_kernel<D(), C()>), grid, dim3(256), 0, s, a);
  });
}

void flashmask_attn_bwd(const FaArgs& a, hipStream_t s) {
  const dim3 gkv((unsigned)(a.b * a.h), (unsigned)cdiv(a.skv, 128));
  const dim3 gq((unsigned)(a.b * a.h), (unsigned)cdiv(a.sq, 128));
  fm_dispatch(a, [&](auto D, auto C) {
    hipLaunchKernelGGL((flashmask_dkv_kernel<D(), C(), false>), gkv, dim3(256), 0, s, a);
    hipLaunchKernelGGL((flashmask_dkv_kernel<D(), C(), true>), gkv, dim3(256), 0, s, a);
    hipLaunchKernelGGL((flashmask_dq_kernel<D(), C()>), gq, dim3(256), 0, s, a);
  });
}

}  // namespace pa
