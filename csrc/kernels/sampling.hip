// Batched token sampling: greedy / temperature / top-k / top-p for a whole
// batch in one launch, one block per row, no sort (docs/KERNELS.md "token
// sampling"; the semantics are on pa::SampleArgs in api.h).
//
// A row becomes monotone unsigned keys (16-bit for bf16, 32-bit for fp32) so
// that the order (logit descending, index ascending) is (key descending,
// index ascending).  Every weight is an integer, rint(2^40 * exp(..)), and a
// function of the key alone, so sums are exact and equal keys weigh the same.
//
//   sweep A   global -> keys (kept in LDS when the row fits), max key and its
//             lowest index.  Greedy rows leave here.
//   sweep Z   Z = sum of weights                       (top_p < 1 only)
//   select    radix select of the kept-set boundary from the top digit down,
//             8 bits per pass: 256-bin {count, weight} LDS histograms over
//             the elements that match the prefix, scanned from the top by
//             one wave.  Leaves the pivot key and how many of its ties stay.
//   final     threads own contiguous slots, so block scans run in index
//             order: tie ranks (u32 scan), kept weights (u64 scan), and the
//             thread whose range holds t = mulhi64(r, Z_S) walks its slots.
//
// Slots: slot = index + shift, with shift chosen so that a 16-byte aligned
// address maps to a slot that is a multiple of EPV.  A slot vector that lies
// inside the row is one 16-byte load; the first and last ones, when ragged,
// are guarded scalar loads (the peeled head and tail).
#include "common.h"
#include "api.h"

namespace pa {
namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / WAVE;
// key bytes a block keeps in LDS (65536 bf16 or 32768 fp32 logits)
constexpr int kResidentBytes = 128 * 1024;
// lane-interleaved histogram copies: lanes of one wave that hit one bin
// spread over this many addresses (a power of two; the macro is for
// measuring other values, docs/KERNELS.md)
#ifndef PA_SAMPLE_HIST_COPIES
#define PA_SAMPLE_HIST_COPIES 8
#endif
constexpr int kHistCopies = PA_SAMPLE_HIST_COPIES;
constexpr u64 kOne = 1ull << 40;

template <int DT> struct SKey;
template <> struct SKey<kBF16> {
  using KT = unsigned short;
  using RT = unsigned short;
  static constexpr int EPV = 8, BITS = 16;
  static __device__ __forceinline__ KT key(RT u) {
    if ((u & 0x7fffu) > 0x7f80u) return 0;            // NaN: lowest
    if (u == 0x8000u) u = 0;                          // -0 == +0
    return (u & 0x8000u) ? (KT)~u : (KT)(u | 0x8000u);
  }
  static __device__ __forceinline__ float value(KT k) {
    unsigned u = (k & 0x8000u) ? (k & 0x7fffu) : (unsigned short)~k;
    return __uint_as_float(u << 16);
  }
};
template <> struct SKey<kF32> {
  using KT = unsigned int;
  using RT = unsigned int;
  static constexpr int EPV = 4, BITS = 32;
  static __device__ __forceinline__ KT key(RT u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0;
    if (u == 0x80000000u) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  static __device__ __forceinline__ float value(KT k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
  }
};

// One slot vector of keys from global memory; slots outside the row read
// nothing and give key 0 (callers mask them by index).
template <int DT>
__device__ __forceinline__ void load_keys(const typename SKey<DT>::RT* row,
                                          int idx0, int v,
                                          typename SKey<DT>::KT* k) {
  using S = SKey<DT>;
  if (idx0 >= 0 && idx0 + S::EPV <= v) {
    struct alignas(16) Vec { typename S::RT e[S::EPV]; };
    Vec raw = *reinterpret_cast<const Vec*>(row + idx0);
#pragma unroll
    for (int e = 0; e < S::EPV; ++e) k[e] = S::key(raw.e[e]);
  } else {
#pragma unroll
    for (int e = 0; e < S::EPV; ++e) {
      int i = idx0 + e;
      k[e] = (i >= 0 && i < v) ? S::key(row[i]) : 0;
    }
  }
}

template <int DT>
__device__ __forceinline__ u64 key_weight(typename SKey<DT>::KT k,
                                          typename SKey<DT>::KT kmax,
                                          float xmax, float c) {
  if (k == kmax) return kOne;
  if (k == 0) return 0;                               // NaN below a real max
  float e = __builtin_amdgcn_exp2f((SKey<DT>::value(k) - xmax) * c);
  return (u64)rintf(e * 0x1p40f);                     // e <= 1: exact product
}

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    T o = __shfl_up(v, off, WAVE);
    if (lane >= off) v += o;
  }
  return v;
}

// Exclusive block scan over the threads in thread order; *total gets the sum.
// `part` holds kSampleWaves entries and is free again after the call.
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* part, T* total) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x >> 6;
  T incl = wave_incl_scan(v, lane);
  if (lane == WAVE - 1) part[wid] = incl;
  __syncthreads();
  T base = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < kSampleWaves; ++i) {
    T p = part[i];
    if (i < wid) base += p;
    sum += p;
  }
  __syncthreads();
  *total = sum;
  return base + incl - v;
}

__device__ __forceinline__ u64 block_max(u64 v, u64* part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    u64 o = __shfl_xor(v, off, WAVE);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 r = 0;
#pragma unroll
  for (int i = 0; i < kSampleWaves; ++i) r = part[i] > r ? part[i] : r;
  __syncthreads();
  return r;
}

// What the selection leaves for the final step.
struct Pivot {
  u32 key;        // kept: key > pivot, or key == pivot with tie rank < ties
  u32 ties;       // 0xffffffff: every tie
  u32 count;      // elements equal to the pivot key
};

template <int DT, bool RESIDENT>
__global__ __launch_bounds__(kSampleThreads) void sample_kernel(SampleArgs a) {
  using S = SKey<DT>;
  using KT = typename S::KT;
  using RT = typename S::RT;
  constexpr int EPV = S::EPV;
  constexpr int NT = kSampleThreads;
  constexpr int KEY_SLOTS = RESIDENT ? kResidentBytes / (int)sizeof(KT) + 2 * EPV : EPV;

  __shared__ __attribute__((aligned(16))) KT keys[KEY_SLOTS];
  __shared__ u64 hist_w[256 * kHistCopies];
  __shared__ u32 hist_c[256 * kHistCopies];
  __shared__ u64 part64[kSampleWaves];
  __shared__ u32 part32[kSampleWaves];
  __shared__ u64 sel_w;             // weight ordered before the selected bin
  __shared__ u32 sel_c, sel_n;      // count before it, count inside it
  __shared__ int sel_bin;

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int v = a.v;
  const RT* row = reinterpret_cast<const RT*>(a.logits) + (long long)b * a.row_stride;
  const int shift = (int)((reinterpret_cast<uintptr_t>(row) / sizeof(RT)) % EPV);
  const int nvec = (shift + v + EPV - 1) / EPV;       // slot vectors

  const float temp = a.temperature[b], top_p = a.top_p[b];
  const int top_k = a.top_k[b];

  // keys of slot vector j: LDS when resident, global (L2) otherwise
  auto get = [&](int j, KT* k) {
    if constexpr (RESIDENT) {
      struct alignas(16) Vec { KT e[EPV]; };
      Vec t = *reinterpret_cast<const Vec*>(&keys[j * EPV]);
#pragma unroll
      for (int e = 0; e < EPV; ++e) k[e] = t.e[e];
    } else {
      load_keys<DT>(row, j * EPV - shift, v, k);
    }
  };

  // ---- sweep A: keys, max key and its lowest index ------------------------
  u64 best = 0;                                       // key << 32 | ~index
  for (int j = tid; j < nvec; j += NT) {
    KT k[EPV];
    load_keys<DT>(row, j * EPV - shift, v, k);
    if constexpr (RESIDENT) {
      struct alignas(16) Vec { KT e[EPV]; };
      Vec t;
#pragma unroll
      for (int e = 0; e < EPV; ++e) t.e[e] = k[e];
      *reinterpret_cast<Vec*>(&keys[j * EPV]) = t;
    }
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      u32 i = (u32)(j * EPV + e - shift);
      u64 cand = ((u64)k[e] << 32) | (u32)~i;
      if (i < (u32)v && cand > best) best = cand;
    }
  }
  best = block_max(best, part64);                     // syncs: keys visible
  const KT kmax = (KT)(best >> 32);
  const int imax = (int)~(u32)best;
  // the first token in the order: greedy, and a kept set of one
  if (!(temp > 0.f) || top_k == 1 || !(top_p > 0.f)) {
    if (tid == 0) a.out[b] = imax;
    return;
  }
  const float xmax = S::value(kmax);
  const float c = 1.44269504088896f / temp;
  const bool use_p = top_p < 1.f;

  Pivot pv = {0u, 0xffffffffu, 0u};                   // keep everything
  if (use_p || top_k > 0) {
    // ---- sweep Z and the weight bound thr = ceil(top_p * Z) ----------------
    u64 thr = ~0ull;
    if (use_p) {
      u64 z = 0;
      for (int j = tid; j < nvec; j += NT) {
        KT k[EPV];
        get(j, k);
#pragma unroll
        for (int e = 0; e < EPV; ++e)
          if ((u32)(j * EPV + e - shift) < (u32)v) z += key_weight<DT>(k[e], kmax, xmax, c);
      }
      u64 total;
      block_excl_scan(z, part64, &total);
      thr = (u64)ceil((double)top_p * (double)total);
    }
    const u32 kk = top_k > 0 ? (u32)top_k : 0xffffffffu;

    // ---- radix select -------------------------------------------------------
    u32 prefix = 0, cb = 0, cn = 0;
    u64 wb = 0;
    bool all = false;
    for (int p = 0; p < S::BITS / 8; ++p) {
      for (int i = tid; i < 256 * kHistCopies; i += NT) { hist_w[i] = 0; hist_c[i] = 0; }
      __syncthreads();
      const int dshift = S::BITS - 8 * (p + 1);
      for (int j = tid; j < nvec; j += NT) {
        KT k[EPV];
        get(j, k);
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          if ((u32)(j * EPV + e - shift) >= (u32)v) continue;
          if (p > 0 && ((u32)k[e] >> (dshift + 8)) != prefix) continue;
          int slot = (((u32)k[e] >> dshift) & 255u) * kHistCopies + (lane & (kHistCopies - 1));
          atomicAdd(&hist_c[slot], 1u);
          if (use_p) {
            u64 w = key_weight<DT>(k[e], kmax, xmax, c);
            if (w) atomicAdd(&hist_w[slot], w);
          }
        }
      }
      __syncthreads();
      if (tid < WAVE) {
        // lane l holds bins 255 - 4l .. 252 - 4l, scanned from the top
        u32 bc[4], csum = 0;
        u64 bw[4], wsum = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          int bin = 255 - (4 * lane + q);
          bc[q] = 0; bw[q] = 0;
#pragma unroll
          for (int r = 0; r < kHistCopies; ++r) {
            bc[q] += hist_c[bin * kHistCopies + r];
            bw[q] += hist_w[bin * kHistCopies + r];
          }
          csum += bc[q]; wsum += bw[q];
        }
        u32 cex = cb + wave_incl_scan(csum, lane) - csum;
        u64 wex = wb + wave_incl_scan(wsum, lane) - wsum;
        int hit = -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bool cross = bc[q] > 0 && (wex + bw[q] >= thr || cex + bc[q] >= kk);
          if (hit < 0 && cross) hit = q;
          if (hit < 0) { cex += bc[q]; wex += bw[q]; }
        }
        u64 m = __ballot(hit >= 0);
        if (m == 0) {
          if (lane == 0) sel_bin = -1;
        } else if (lane == __ffsll((long long)m) - 1) {
          sel_bin = 255 - (4 * lane + hit);
          sel_w = wex; sel_c = cex; sel_n = bc[hit];
        }
      }
      __syncthreads();
      const int bin = sel_bin;
      if (bin < 0) { all = true; break; }             // nothing crosses: keep all
      prefix = (prefix << 8) | (u32)bin;
      wb = sel_w; cb = sel_c; cn = sel_n;   // rewritten two barriers from here
    }
    if (!all) {
      // ties m = 0, 1, .. of the pivot sit behind weight wb + m * w and rank
      // cb + m; wb < thr and cb < kk hold by construction
      const u64 w = key_weight<DT>((KT)prefix, kmax, xmax, c);
      u64 by_p = (w == 0 || !use_p) ? cn : (thr - wb - 1) / w + 1;
      u64 by_k = (u64)kk - cb;
      u64 n = by_p < by_k ? by_p : by_k;
      pv.key = prefix;
      pv.count = cn;
      pv.ties = n >= cn ? 0xffffffffu : (u32)n;
    }
  }

  // ---- final step: contiguous slots per thread, scans in index order --------
  const int per = ((nvec + NT - 1) / NT);             // slot vectors per thread
  const int j0 = tid * per, j1 = min(j0 + per, nvec);
  u32 tie_base = 0;
  if (pv.ties != 0xffffffffu) {
    u32 n = 0;
    for (int j = j0; j < j1; ++j) {
      KT k[EPV];
      get(j, k);
#pragma unroll
      for (int e = 0; e < EPV; ++e)
        n += ((u32)(j * EPV + e - shift) < (u32)v && (u32)k[e] == pv.key) ? 1u : 0u;
    }
    u32 total;
    tie_base = block_excl_scan(n, part32, &total);
  }
  // kept weight of one element; advances the running tie rank
  auto kept_weight = [&](KT k, u32 i, u32& rank) -> u64 {
    if (i >= (u32)v || (u32)k < pv.key) return 0;
    if ((u32)k == pv.key && rank++ >= pv.ties) return 0;
    return key_weight<DT>(k, kmax, xmax, c);
  };
  u64 mine = 0;
  u32 rank = tie_base;
  for (int j = j0; j < j1; ++j) {
    KT k[EPV];
    get(j, k);
#pragma unroll
    for (int e = 0; e < EPV; ++e) mine += kept_weight(k[e], (u32)(j * EPV + e - shift), rank);
  }
  u64 zs;
  const u64 before = block_excl_scan(mine, part64, &zs);
  u64 r;
  if (a.rand_bits) {
    r = (u64)a.rand_bits[b];
  } else {
    uintx4 x = philox10((u64)a.seed[b], (u64)a.offset[b]);
    r = ((u64)x[0] << 32) | x[1];
  }
  const u64 t = __umul64hi(r, zs);                    // 0 <= t < zs
  if (t >= before && t - before < mine) {             // exactly one thread
    u64 acc = before;
    rank = tie_base;
    int pick = -1;
    for (int j = j0; j < j1 && pick < 0; ++j) {
      KT k[EPV];
      get(j, k);
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        u32 i = (u32)(j * EPV + e - shift);
        acc += kept_weight(k[e], i, rank);
        if (pick < 0 && acc > t) pick = (int)i;
      }
    }
    a.out[b] = pick;
  }
}

template <int DT>
void launch(const SampleArgs& a, hipStream_t s) {
  const bool resident = (int64_t)a.v * (int64_t)sizeof(typename SKey<DT>::KT) <= kResidentBytes;
  if (resident)
    hipLaunchKernelGGL((sample_kernel<DT, true>), dim3(a.b), dim3(kSampleThreads), 0, s, a);
  else
    hipLaunchKernelGGL((sample_kernel<DT, false>), dim3(a.b), dim3(kSampleThreads), 0, s, a);
}

}  // namespace

void sample_tokens(const SampleArgs& a, hipStream_t s) {
  if (a.dtype == kBF16) launch<kBF16>(a, s);
  else launch<kF32>(a, s);
}

}  // namespace pa
