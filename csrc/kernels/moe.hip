// MoE routing kernels for gfx950: fused top-k gate + deterministic
// capacity slot assignment, and the collision-free slot maps of the fused
// dispatch / combine path (moe_route, row movers in moe_permute.hip).
//
// Reference role: paddle/phi/kernels/gpu/{assign_pos,number_count,
// limit_by_capacity,prune_gate_by_capacity}_kernel.cu + the gate math in
// incubate/distributed/models/moe/gate/gshard_gate.py -- re-derived as
// two wave64 kernels instead of the reference's kernel-per-step chain:
//   * gate: one wave per token (E <= 64: one expert logit per lane) does
//     softmax + top-k + load-balance stats in registers
//   * assign: one wave per (expert, k) walks tokens in 64-chunks using
//     __ballot + popc prefix -- positions follow token order exactly like
//     the reference's cumsum (deterministic capacity dropping), no sort
//   * route: one block per expert owns the whole (kk, t) sequence of its
//     expert, so positions run on across kk (GShard order: every first
//     choice before every second choice) and no two (t, kk) share a slot
#include "common.h"
#include "api.h"
#include <type_traits>

namespace pa {

// logits [T, E] fp32 (E <= 64), k <= 4
// outputs: topv [T,k] f32 (softmax probs), topi [T,k] i32,
//          me [E] f32 (+= mean prob), ce [E] f32 (+= top1 counts / T)
__global__ void moe_gate_kernel(const float* __restrict__ logits,
                                float* __restrict__ topv, int* __restrict__ topi,
                                float* __restrict__ me, float* __restrict__ ce,
                                long long T, int E, int K) {
  const long long t = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (t >= T) return;
  float lg = (lane < E) ? logits[t * E + lane] : -1e30f;
  // softmax over the wave
  float mx = wave_reduce(lg, MaxOp());
  float ex = (lane < E) ? __expf(lg - mx) : 0.f;
  float den = wave_reduce(ex, SumOp());
  float p = ex / den;
  if (lane < E) atomicAdd(&me[lane], p / (float)T);
  float pw = p;
  for (int kk = 0; kk < K; ++kk) {
    float best = wave_reduce(pw, MaxOp());
    // first lane holding the max wins
    unsigned long long win = __ballot(pw == best);
    int win_lane = (int)__ffsll((long long)win) - 1;
    if (lane == 0) {
      topv[t * K + kk] = best;
      topi[t * K + kk] = win_lane;
      if (kk == 0) atomicAdd(&ce[win_lane], 1.f / (float)T);
    }
    if (lane == win_lane) pw = -1.f;   // remove from next round
  }
}

// topi [T, k] i32 -> slot_of [T, k] i32 (expert*cap + pos, or -1 dropped),
// counts [E] i32.  grid = E * K waves; wave w handles (expert e, slot kk).
__global__ void moe_assign_kernel(const int* __restrict__ topi,
                                  int* __restrict__ slot_of,
                                  int* __restrict__ counts,
                                  long long T, int E, int K, int cap) {
  const int w = ((int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= E * K) return;
  const int e = w / K, kk = w % K;
  int base = 0;
  for (long long t0 = 0; t0 < T; t0 += 64) {
    long long t = t0 + lane;
    bool match = (t < T) && (topi[t * K + kk] == e);
    unsigned long long mask = __ballot(match);
    if (match) {
      int pos = base + __popcll(mask & ((1ull << lane) - 1));
      slot_of[t * K + kk] = (pos < cap) ? (e * cap + pos) : -1;
    }
    base += __popcll(mask);
  }
  if (lane == 0) atomicAdd(&counts[e], base);
}

// topi [T, K] i32 -> slot_of [T, K], src_of [E * cap], counts [E], every
// element written here by plain stores (no initialisation, no atomics).
// Block e walks the sequence i = kk * T + t in 64-chunks; pos(t, kk) is the
// number of earlier entries of the sequence that chose e.  NW == 1 is one
// wave carrying `base` through the walk.  NW > 1 cuts the chunk list into NW
// consecutive runs: every wave counts its run, the counts meet in LDS once,
// and each wave walks its run again from the sum of the runs before it.
// Block 0 also writes -1 for expert ids outside [0, E).
template <int NW>
__global__ __launch_bounds__(NW * 64) void moe_route_kernel(
    const int* __restrict__ topi, int* __restrict__ slot_of,
    int* __restrict__ src_of, int* __restrict__ counts, int T, int E, int K,
    int cap) {
  __shared__ int wcount[NW];
  const int e = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nch = (T + 63) >> 6;           // 64-chunks per kk
  const int total = nch * K;
  const int per = (total + NW - 1) / NW;
  const int c0 = min(total, wv * per), c1 = min(total, c0 + per);
  const unsigned long long below = (1ull << lane) - 1;
  int base = 0, n_e = 0;
  if (NW > 1) {
    int n = 0;
    for (int c = c0; c < c1; ++c) {
      const int kk = c / nch, t = ((c - kk * nch) << 6) + lane;
      n += __popcll(__ballot(t < T && topi[t * K + kk] == e));
    }
    if (lane == 0) wcount[wv] = n;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      if (i < wv) base += wcount[i];
      n_e += wcount[i];
    }
  }
  for (int c = c0; c < c1; ++c) {
    const int kk = c / nch, t = ((c - kk * nch) << 6) + lane;
    const int id = (t < T) ? topi[t * K + kk] : e + 1;
    const bool match = (t < T) && id == e;
    const unsigned long long mask = __ballot(match);
    if (match) {
      const int pos = base + __popcll(mask & below);
      if (pos < cap) {
        slot_of[t * K + kk] = e * cap + pos;
        src_of[e * cap + pos] = t * K + kk;
      } else {
        slot_of[t * K + kk] = -1;
      }
    }
    if (e == 0 && t < T && (unsigned)id >= (unsigned)E) slot_of[t * K + kk] = -1;
    base += __popcll(mask);
  }
  if (NW == 1) n_e = base;
  for (int p = min(n_e, cap) + (int)threadIdx.x; p < cap; p += NW * 64)
    src_of[e * cap + p] = -1;
  if (threadIdx.x == 0) counts[e] = n_e;
}

// Compact (dropless) route: topi [T, K] -> slot_of [T, K], src_of [T * K],
// offsets [E + 1], every element written by plain stores.  Block e walks the
// same sequence as moe_route_kernel twice.  The first walk counts, per wave
// run, the entries of expert e, the valid entries below e and all valid
// entries: topi is L2-resident, so each block forms its own prefix over the
// experts before it and no second launch or atomic is needed.  The second
// walk hands out offsets[e] + pos.  All blocks share the -1 tail of src_of.
template <int NW>
__global__ __launch_bounds__(NW * 64) void moe_route_ragged_kernel(
    const int* __restrict__ topi, int* __restrict__ slot_of,
    int* __restrict__ src_of, int* __restrict__ offsets, int T, int E, int K) {
  __shared__ int wmine[NW], wbelow[NW], wvalid[NW];
  const int e = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nch = (T + 63) >> 6;
  const int total = nch * K;
  const int per = (total + NW - 1) / NW;
  const int c0 = min(total, wv * per), c1 = min(total, c0 + per);
  const unsigned long long lower = (1ull << lane) - 1;
  int nm = 0, nb = 0, nv = 0;
  for (int c = c0; c < c1; ++c) {
    const int kk = c / nch, t = ((c - kk * nch) << 6) + lane;
    const int id = (t < T) ? topi[t * K + kk] : -1;
    nm += __popcll(__ballot(id == e));
    nb += __popcll(__ballot((unsigned)id < (unsigned)e));
    nv += __popcll(__ballot((unsigned)id < (unsigned)E));
  }
  if (lane == 0) { wmine[wv] = nm; wbelow[wv] = nb; wvalid[wv] = nv; }
  __syncthreads();
  int base = 0, below = 0, valid = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    if (i < wv) base += wmine[i];
    below += wbelow[i];
    valid += wvalid[i];
  }
  base += below;
  for (int c = c0; c < c1; ++c) {
    const int kk = c / nch, t = ((c - kk * nch) << 6) + lane;
    const int id = (t < T) ? topi[t * K + kk] : e;
    const bool match = (t < T) && id == e;
    const unsigned long long mask = __ballot(match);
    if (match) {
      const int slot = base + __popcll(mask & lower);
      slot_of[t * K + kk] = slot;
      src_of[slot] = t * K + kk;
    }
    if (e == 0 && t < T && (unsigned)id >= (unsigned)E) slot_of[t * K + kk] = -1;
    base += __popcll(mask);
  }
  for (long long p = valid + (long long)e * NW * 64 + threadIdx.x; p < (long long)T * K;
       p += (long long)E * NW * 64)
    src_of[p] = -1;
  if (threadIdx.x == 0) {
    offsets[e] = below;
    if (e == E - 1) offsets[E] = valid;
  }
}

void moe_route_ragged(const int* topi, int* slot_of, int* src_of, int* offsets,
                      int64_t t, int64_t e, int64_t k, hipStream_t s) {
  const int64_t chunks = ((t + 63) / 64) * k;
  auto go = [&](auto NW) {
    hipLaunchKernelGGL((moe_route_ragged_kernel<NW()>), dim3((unsigned)e),
                       dim3(NW() * 64), 0, s, topi, slot_of, src_of, offsets,
                       (int)t, (int)e, (int)k);
  };
  if (chunks <= 4) go(std::integral_constant<int, 1>{});
  else if (chunks <= 64) go(std::integral_constant<int, 4>{});
  else go(std::integral_constant<int, 16>{});
}

void moe_gate_topk(const float* logits, float* topv, int* topi, float* me,
                   float* ce, int64_t t, int64_t e, int64_t k, hipStream_t s) {
  long long waves = t;
  dim3 g((unsigned)hmin<long long>((waves * 64 + 255) / 256, 1 << 30));
  hipLaunchKernelGGL(moe_gate_kernel, g, dim3(256), 0, s, logits, topv, topi,
                     me, ce, t, (int)e, (int)k);
}

void moe_assign_slots(const int* topi, int* slot_of, int* counts, int64_t t,
                      int64_t e, int64_t k, int64_t cap, hipStream_t s) {
  long long waves = e * k;
  dim3 g((unsigned)((waves * 64 + 255) / 256));
  hipLaunchKernelGGL(moe_assign_kernel, g, dim3(256), 0, s, topi, slot_of,
                     counts, t, (int)e, (int)k, (int)cap);
}

// block_waves: 1, 4 or 16 waves per expert block; 0 picks by the length of
// the walk (measured at T = 8192, docs/KERNELS.md "MoE dispatch / combine")
void moe_route(const int* topi, int* slot_of, int* src_of, int* counts,
               int64_t t, int64_t e, int64_t k, int64_t cap, int block_waves,
               hipStream_t s) {
  if (block_waves == 0) {
    const int64_t chunks = ((t + 63) / 64) * k;
    block_waves = chunks <= 4 ? 1 : chunks <= 64 ? 4 : 16;
  }
  auto go = [&](auto NW) {
    hipLaunchKernelGGL((moe_route_kernel<NW()>), dim3((unsigned)e),
                       dim3(NW() * 64), 0, s, topi, slot_of, src_of, counts,
                       (int)t, (int)e, (int)k, (int)cap);
  };
  if (block_waves == 1) go(std::integral_constant<int, 1>{});
  else if (block_waves == 4) go(std::integral_constant<int, 4>{});
  else go(std::integral_constant<int, 16>{});
}

}  // namespace pa
