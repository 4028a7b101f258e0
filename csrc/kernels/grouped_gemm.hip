// Ragged grouped bf16 GEMM for gfx950: the expert GEMMs of a dropless MoE
// layer.  R = T * K rows are sorted by expert; group e owns the rows
// [offsets[e], offsets[e + 1]) and the offsets stay on the device (no host
// read, graph-capturable).  fp32 accumulate, bf16 out, three forms:
//   NN  C[r, :] = A[r, :] . B[g(r)] (+ bias[g(r), :])   B [E, K, N]   forward
//   NT  C[r, :] = A[r, :] . B[g(r)]^T                   B [E, N, K]   dgrad
//   TN  C[e] = sum_{r in group e} A[r, :]^T (x) B[r, :] C [E, M, N]   wgrad
// The stored weights w1 [E, h, I], w2 [E, I, h] serve all three forms in
// place; no transposed copy exists anywhere.
//
// Geometry.  Block tile 128 x 128, K-step 64, 4 waves (2 x 2), 64 x 64 per
// wave = acc[4][4] mfma_f32_16x16x32_bf16 fragments.  Two {A, B} buffers of
// 16 KiB per operand = 64 KiB LDS, two blocks per CU: tile t + 1 is in flight
// (DMA) while tile t is computed, one barrier per K-tile.  128 rows, not the
// 256 of gemm.hip: the mean group of the measured layer is 256 rows, and the
// last m-tile of a group is on average half empty, so the MFMA waste per
// group is ~BM/2 rows: 64 of 64+64 (50 %) at a mean group of 64, 64 of 320
// (20 %) at 256 and 64 of 1088 (6 %) at 1024; BM = 256 would waste 67 %, 33 %
// and 11 %.  BM = 64 halves the waste again but doubles the B traffic per
// FLOP, and the B panel is the large operand here.
//
// The MFMA computes C^T: the B fragment goes in as the A operand and the A
// fragment as the B operand (both hold [non-k = l16][k = 8 * lg + 0..7]), so
// lane (l16, lg) ends with C[m = l16][n = 4 * lg + 0..3] and stores 8 bytes
// of one row instead of four 2-byte pieces of four rows.
//
// LDS images.  Every operand tile lands in its natural row-major image by
// global_load_lds (16 B per lane, lane-linear target, so the XOR sits on the
// source column: the lane filling chunk position c of row r fetches chunk
// c ^ swz(r)).  Bank rule as in fa_common.h: a 256-byte bank row of 16 slots;
// ds_read_b128 conflicts inside its 16-lane groups {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} (+32), ds_read_b64_tr_b16 inside a 32-lane half.
//   kc image [128][64] (k contiguous: A of NN / NT, B of NT), 128-byte rows,
//     chunk ^ (row & 7), read by rows.  Two rows share a bank row: slot =
//     8 * (row & 1) + (chunk ^ (row & 7)).  A group reads rows {0-3, 12-15} at
//     chunk c and rows {4-11} at c ^ 1.  In the half row & 1 = 0 that is
//     c ^ {0, 2, 4, 6} and c ^ 1 ^ {4, 6, 0, 2} = c ^ {5, 7, 1, 3}: eight
//     different slots, and the same in the other half: 16 slots, no conflict.
//   km image [64][128] (k along rows: B of NN, both operands of TN), 256-byte
//     rows = one bank row, chunk ^ km_swz(row), read by columns.  A 32-lane
//     half of a transposed read takes rows 8g + {0..3} of two 16-lane groups
//     g, g + 1, 32 bytes (one chunk pair) per row: the pair index is XORed
//     with (row & 3) << 1 | (row >> 3) & 1, eight different pairs for the
//     eight rows.  Rows r + 4 (second half of a fragment) and r + 32 (next
//     k-step) keep the XOR, so they are immediate offsets from one address
//     register per fragment.  This is the D = 128 image of fa_bwd_dkv_kernel.
//
// Ragged rows.  NN / NT: a tile map (one prep launch per route) names the
// (group, first row) of every m-tile.  A row past the end of a group is a row
// of the next group: loaded (row address clamped to R - 1), computed, never
// stored, so one unguarded body serves every m-tile.  A pseudo-group E covers
// the rows [offsets[E], R) of invalid ids; its tiles write zeros.  TN: block
// (e, m-tile, n-tile) walks its group in row order; the last, partial k-tile
// is staged by guarded loads with zero fill; an empty group stores zeros.  No
// split of a group across blocks and no atomics: results do not depend on
// dispatch order.  Offsets are clamped to [0, R] and never trusted.
//
// Schedule.  The linear block index is cut into contiguous chunks per XCD
// (as gemm_tile_origin does).  NN / NT then walk bands of 4 m-tiles with the
// n-tile slower, so the blocks resident on an XCD at one time cover a few
// neighbouring m-tiles -- in map order those belong to one or two experts --
// and share that expert's B panel in L2.  TN orders blocks by expert first.
#include "common.h"
#include "api.h"

namespace pa {

namespace {

constexpr int BM = kGroupedGemmBM, BN = 128, BK = 64, NTHR = 256;
constexpr int TILE = 128 * 64 * 2;   // bytes of one operand tile
static_assert(BM == 128, "the wave layout is 2 x 2 x (64 x 64)");

struct GGParams {
  const short *a, *b;
  short* c;
  const short* bias;
  const int *offsets, *map;
  int R, E, d0, N, map_tiles;   // d0: K (NN / NT) or M (TN)
  long long lda, ldb, ldc, ldbias, b_gs, c_gs;
};

typedef __attribute__((address_space(1))) const unsigned int* gptr_t;
typedef __attribute__((address_space(3))) unsigned int* lptr_t;

__device__ __forceinline__ void gg_range(const int* off, int e, int R, int& lo, int& hi) {
  const int o0 = off[e], o1 = off[e + 1];
  lo = min(max(o0, 0), R);
  hi = min(max(max(o1, o0), 0), R);
}

__device__ __forceinline__ int gg_xcd_chunk(int orig, int nwg) {
  const int nx = 8, q = nwg / nx, rr = nwg % nx;
  const int xcd = orig % nx, pos = orig / nx;
  return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + pos;
}

__device__ __forceinline__ unsigned km_swz(unsigned row) {
  return ((row & 3u) << 2) | (((row >> 3) & 1u) << 1);
}
__device__ __forceinline__ unsigned km_off(unsigned row, unsigned ch) {
  return row * 256 + ((ch ^ km_swz(row)) << 4);
}

// Fragment reads.  Inline asm that ends in its own lgkmcnt(0): the compiler
// then neither waits for the DMA of the next tile in front of an LDS read nor
// touches a fragment register before its data has arrived.  EXEC is all ones
// at every call.  kc: four row fragments 16 rows (2048 bytes) apart from one
// address; km: four column fragments, rows +4 are 1024 bytes on.
__device__ __forceinline__ void gg_read_kc_kc(shortx8 (&x)[4], shortx8 (&y)[4],
                                              unsigned ax, unsigned ay) {
  asm volatile(
      "ds_read_b128 %0, %8\n\t"
      "ds_read_b128 %1, %8 offset:2048\n\t"
      "ds_read_b128 %2, %8 offset:4096\n\t"
      "ds_read_b128 %3, %8 offset:6144\n\t"
      "ds_read_b128 %4, %9\n\t"
      "ds_read_b128 %5, %9 offset:2048\n\t"
      "ds_read_b128 %6, %9 offset:4096\n\t"
      "ds_read_b128 %7, %9 offset:6144\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]),
        "=&v"(y[0]), "=&v"(y[1]), "=&v"(y[2]), "=&v"(y[3])
      : "v"(ax), "v"(ay)
      : "memory");
}

template <int LO>
__device__ __forceinline__ void gg_read_kc_km(shortx8 (&x)[4], shortx8 (&y)[4],
                                              unsigned ax, const unsigned (&ay)[4]) {
  shortx4 l0, h0, l1, h1, l2, h2, l3, h3;
  asm volatile(
      "ds_read_b128 %0, %12\n\t"
      "ds_read_b128 %1, %12 offset:2048\n\t"
      "ds_read_b128 %2, %12 offset:4096\n\t"
      "ds_read_b128 %3, %12 offset:6144\n\t"
      "ds_read_b64_tr_b16 %4, %13 offset:%17\n\t"
      "ds_read_b64_tr_b16 %5, %13 offset:%18\n\t"
      "ds_read_b64_tr_b16 %6, %14 offset:%17\n\t"
      "ds_read_b64_tr_b16 %7, %14 offset:%18\n\t"
      "ds_read_b64_tr_b16 %8, %15 offset:%17\n\t"
      "ds_read_b64_tr_b16 %9, %15 offset:%18\n\t"
      "ds_read_b64_tr_b16 %10, %16 offset:%17\n\t"
      "ds_read_b64_tr_b16 %11, %16 offset:%18\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]),
        "=&v"(l0), "=&v"(h0), "=&v"(l1), "=&v"(h1), "=&v"(l2), "=&v"(h2),
        "=&v"(l3), "=&v"(h3)
      : "v"(ax), "v"(ay[0]), "v"(ay[1]), "v"(ay[2]), "v"(ay[3]), "n"(LO),
        "n"(LO + 1024)
      : "memory");
  y[0] = __builtin_shufflevector(l0, h0, 0, 1, 2, 3, 4, 5, 6, 7);
  y[1] = __builtin_shufflevector(l1, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  y[2] = __builtin_shufflevector(l2, h2, 0, 1, 2, 3, 4, 5, 6, 7);
  y[3] = __builtin_shufflevector(l3, h3, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int LO>
__device__ __forceinline__ void gg_read_km(shortx8 (&y)[4], const unsigned (&ay)[4]) {
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
      : "v"(ay[0]), "v"(ay[1]), "v"(ay[2]), "v"(ay[3]), "n"(LO), "n"(LO + 1024)
      : "memory");
  y[0] = __builtin_shufflevector(l0, h0, 0, 1, 2, 3, 4, 5, 6, 7);
  y[1] = __builtin_shufflevector(l1, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  y[2] = __builtin_shufflevector(l2, h2, 0, 1, 2, 3, 4, 5, 6, 7);
  y[3] = __builtin_shufflevector(l3, h3, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---------------------------------------------------------------------------
// prep: offsets -> tile map of the ragged-M forms.  One block; thread e owns
// group e.  map[2 i], map[2 i + 1] = (group, first row) of m-tile i in group
// order, the pseudo-group E of the invalid tail last, (-1, -1) after it; every
// element is written.  The scan saturates at map_tiles, so malformed offsets
// (overlapping groups) cannot index past the map.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void grouped_gemm_plan_kernel(
    const int* __restrict__ offsets, int* __restrict__ map, int R, int E,
    int map_tiles) {
  __shared__ int scan[1024];
  const int tid = threadIdx.x;
  int lo = 0, nt = 0;
  if (tid < E) {
    int hi;
    gg_range(offsets, tid, R, lo, hi);
    nt = (hi - lo + BM - 1) / BM;
  }
  scan[tid] = min(nt, map_tiles);
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] = min(scan[tid] + v, map_tiles);
    __syncthreads();
  }
  const int base = tid > 0 ? scan[tid - 1] : 0;
  const int total = scan[1023];
  for (int j = 0; j < nt && base + j < map_tiles; ++j) {
    map[2 * (base + j)] = tid;
    map[2 * (base + j) + 1] = lo + j * BM;
  }
  const int tlo = min(max(offsets[E], 0), R);
  const int ntail = (R - tlo + BM - 1) / BM;
  for (int j = tid; j < ntail && total + j < map_tiles; j += 1024) {
    map[2 * (total + j)] = E;
    map[2 * (total + j) + 1] = tlo + j * BM;
  }
  for (int i = min(total + ntail, map_tiles) + tid; i < map_tiles; i += 1024) {
    map[2 * i] = -1;
    map[2 * i + 1] = -1;
  }
}

// ---------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------
template <int FORM, bool BIAS>
__global__ __launch_bounds__(NTHR, 2) void grouped_gemm_kernel(GGParams p) {
  constexpr bool TN = FORM == kGroupedTN;
  constexpr bool A_KC = !TN;                  // A image has k contiguous
  constexpr bool B_KC = FORM == kGroupedNT;   // B image has k contiguous
  __shared__ __attribute__((aligned(16))) char lds[4 * TILE];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1, l16 = lane & 15, lg = lane >> 4;
  const int L = gg_xcd_chunk((int)blockIdx.x, (int)gridDim.x);
  const int ntn = (p.N + BN - 1) / BN;

  // ---- which tile ---------------------------------------------------------
  int g, row0, col0, lo, hi, nfull, nkt;
  if (!TN) {
    constexpr int GM = 4;
    const int band = L / (GM * ntn), rem = L - band * (GM * ntn);
    const int gmb = min(GM, p.map_tiles - band * GM);
    const int mt = band * GM + rem % gmb;
    col0 = (rem / gmb) * BN;
    g = p.map[2 * mt];
    row0 = p.map[2 * mt + 1];
    if ((unsigned)g > (unsigned)p.E || (unsigned)row0 >= (unsigned)p.R) return;
    if (g == p.E) {
      // rows of invalid ids: zeros
      const int nch = min(BN, p.N - col0) >> 3;
      const shortx8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int i = tid; i < BM * 16; i += NTHR) {
        const int r = i >> 4, ch = i & 15;
        if (row0 + r < p.R && ch < nch)
          *reinterpret_cast<shortx8*>(p.c + (long long)(row0 + r) * p.ldc + col0 + ch * 8) = z;
      }
      return;
    }
    gg_range(p.offsets, g, p.R, lo, hi);
    if (row0 >= hi) return;
    nfull = nkt = p.d0 / BK;
  } else {
    const int mtm = (p.d0 + BM - 1) / BM;
    g = L / (mtm * ntn);
    const int rem = L - g * (mtm * ntn);
    row0 = (rem % mtm) * BM;                  // m0
    col0 = (rem / mtm) * BN;                  // n0
    gg_range(p.offsets, g, p.R, lo, hi);
    nfull = (hi - lo) >> 6;
    nkt = nfull + (((hi - lo) & 63) != 0);
  }

  // ---- DMA source pointers: 4 rounds of 256 threads x 16 bytes per tile ----
  // kc image: chunk position tid & 7 of row 32 it + (tid >> 3);
  // km image: chunk position tid & 15 of row 16 it + (tid >> 4).
  const int r_kc = tid >> 3, ch_kc = (tid & 7) ^ ((tid >> 3) & 7);
  const int r_km = tid >> 4, ch_km = (tid & 15) ^ (int)km_swz(tid >> 4);
  const short* aptr[4];
  const short* bptr[4];
  long long astep, bstep;
  {
    // column of a km image's chunk, wrapped into the last whole 64-column slab
    auto km_col = [](int c0, int ch, int lim) {
      const int c = c0 + ch * 8;
      return c < lim ? c : c - 64;
    };
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      if (A_KC) {
        const int r = min(row0 + r_kc + 32 * it, p.R - 1);
        aptr[it] = p.a + (long long)r * p.lda + ch_kc * 8;
      } else {
        aptr[it] = p.a + (long long)(lo + r_km + 16 * it) * p.lda +
                   km_col(row0, ch_km, p.d0);
      }
      if (FORM == kGroupedNN) {
        bptr[it] = p.b + (long long)g * p.b_gs + (long long)(r_km + 16 * it) * p.ldb +
                   km_col(col0, ch_km, p.N);
      } else if (FORM == kGroupedNT) {
        const int n = min(col0 + r_kc + 32 * it, p.N - 1);
        bptr[it] = p.b + (long long)g * p.b_gs + (long long)n * p.ldb + ch_kc * 8;
      } else {
        bptr[it] = p.b + (long long)(lo + r_km + 16 * it) * p.ldb +
                   km_col(col0, ch_km, p.N);
      }
    }
    astep = A_KC ? BK : BK * p.lda;
    bstep = B_KC ? BK : BK * p.ldb;
  }

  auto stage_dma = [&](int buf) {
    char* base = lds + buf * 2 * TILE + wid * 1024;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      __builtin_amdgcn_global_load_lds((gptr_t)aptr[it], (lptr_t)(base + it * 4096), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)bptr[it], (lptr_t)(base + TILE + it * 4096), 16, 0, 0);
      aptr[it] += astep;
      bptr[it] += bstep;
    }
  };
  // TN's last, partial k-tile: rows at or past the group's end are zeros
  [[maybe_unused]] auto stage_tail = [&](int buf) {
    char* base = lds + buf * 2 * TILE;
    const int valid = (hi - lo) & 63;
    const long long r0 = (long long)lo + (long long)nfull * BK;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int pos = it * NTHR + tid, row = pos >> 4, ch = pos & 15;
      int ca = row0 + ch * 8, cb = col0 + ch * 8;
      if (ca >= p.d0) ca -= 64;
      if (cb >= p.N) cb -= 64;
      shortx8 va = {0, 0, 0, 0, 0, 0, 0, 0}, vb = {0, 0, 0, 0, 0, 0, 0, 0};
      if (row < valid) {
        va = *reinterpret_cast<const shortx8*>(p.a + (r0 + row) * p.lda + ca);
        vb = *reinterpret_cast<const shortx8*>(p.b + (r0 + row) * p.ldb + cb);
      }
      const unsigned o = km_off(row, ch);
      *reinterpret_cast<shortx8*>(base + o) = va;
      *reinterpret_cast<shortx8*>(base + TILE + o) = vb;
    }
  };
  auto stage = [&](int t, int buf) {
    if (!TN || t < nfull) stage_dma(buf); else stage_tail(buf);
  };

  // ---- fragment addresses ---------------------------------------------------
  const unsigned lds_a = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  const unsigned tr_q = l16 >> 2, tr_p = l16 & 3;
  // kc: row 64 w + 16 f + l16, chunk (4 ks + lg) ^ (l16 & 7); one register per ks
  auto kc_addr = [&](int w, int ks) {
    return (unsigned)((w * 64 + l16) * 128 + (((ks * 4 + lg) ^ (l16 & 7)) << 4));
  };
  // km: row 8 lg + tr_q, the lane's 8 bytes of column tile 4 w + f
  auto km_addr = [&](int w, int f) {
    return km_off(8 * lg + tr_q, 2 * (4 * w + f) + (tr_p >> 1)) + ((tr_p & 1u) << 3);
  };
  unsigned a_kc[2], b_kc[2], a_km[4], b_km[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    a_kc[i] = lds_a + kc_addr(wr, i);
    b_kc[i] = lds_a + TILE + kc_addr(wc, i);
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    a_km[f] = lds_a + km_addr(wr, f);
    b_km[f] = lds_a + TILE + km_addr(wc, f);
  }

  floatx4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = {0.f, 0.f, 0.f, 0.f};

  auto mma = [&](const shortx8 (&af)[4], const shortx8 (&bf)[4]) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = mfma_bf16(bf[n], af[m], acc[m][n]);
  };
  auto compute = [&](int buf) {
    const unsigned bo = buf * 2 * TILE;
    shortx8 af[4], bf[4];
    if (FORM == kGroupedNT) {
      gg_read_kc_kc(af, bf, a_kc[0] + bo, b_kc[0] + bo);
      mma(af, bf);
      gg_read_kc_kc(af, bf, a_kc[1] + bo, b_kc[1] + bo);
      mma(af, bf);
    } else if (FORM == kGroupedNN) {
      const unsigned bb[4] = {b_km[0] + bo, b_km[1] + bo, b_km[2] + bo, b_km[3] + bo};
      gg_read_kc_km<0>(af, bf, a_kc[0] + bo, bb);
      mma(af, bf);
      gg_read_kc_km<8192>(af, bf, a_kc[1] + bo, bb);
      mma(af, bf);
    } else {
      const unsigned aa[4] = {a_km[0] + bo, a_km[1] + bo, a_km[2] + bo, a_km[3] + bo};
      const unsigned bb[4] = {b_km[0] + bo, b_km[1] + bo, b_km[2] + bo, b_km[3] + bo};
      gg_read_km<0>(af, aa);
      gg_read_km<0>(bf, bb);
      mma(af, bf);
      gg_read_km<8192>(af, aa);
      gg_read_km<8192>(bf, bb);
      mma(af, bf);
    }
  };

  // ---- main loop: tile t + 1 lands while tile t is computed ------------------
  if (nkt > 0) {
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
  }
  for (int t = 0; t < nkt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nkt) stage(t + 1, cur ^ 1);
    compute(cur);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: lane holds C[m = l16][n = 4 lg + 0..3] of each fragment ----
  const int ncol = col0 + wc * 64;
  if (ncol >= p.N) return;                     // wave-uniform 64-column slab
  if (TN && row0 + wr * 64 >= p.d0) return;
  short* cbase = p.c + (TN ? (long long)g * p.c_gs : 0);
  const int row_end = TN ? p.d0 : hi;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int col = ncol + n * 16 + 4 * lg;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (BIAS) {
      const shortx4 b4 = *reinterpret_cast<const shortx4*>(p.bias + (long long)g * p.ldbias + col);
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[r] = bf2f(b4[r]);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int row = row0 + wr * 64 + m * 16 + l16;
      if (row >= row_end) continue;
      shortx4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = f2bf(acc[m][n][r] + bv[r]);
      *reinterpret_cast<shortx4*>(cbase + (long long)row * p.ldc + col) = o;
    }
  }
}

}  // namespace

int64_t grouped_gemm_map_tiles(int64_t rows, int64_t groups) {
  return (rows + BM - 1) / BM + groups + 1;
}

void grouped_gemm_plan(const int* offsets, int* tile_map, int64_t rows,
                       int64_t groups, hipStream_t s) {
  hipLaunchKernelGGL(grouped_gemm_plan_kernel, dim3(1), dim3(1024), 0, s,
                     offsets, tile_map, (int)rows, (int)groups,
                     (int)grouped_gemm_map_tiles(rows, groups));
}

void grouped_gemm_bf16(const GroupedGemmArgs& a, hipStream_t s) {
  if (a.rows == 0) return;
  GGParams p;
  p.a = (const short*)a.a; p.b = (const short*)a.b; p.c = (short*)a.c;
  p.bias = (const short*)a.bias;
  p.offsets = a.offsets; p.map = a.tile_map;
  p.R = (int)a.rows; p.E = (int)a.groups; p.N = (int)a.n;
  p.d0 = (int)(a.form == kGroupedTN ? a.m : a.k);
  p.map_tiles = (int)grouped_gemm_map_tiles(a.rows, a.groups);
  p.lda = a.lda; p.ldb = a.ldb; p.ldc = a.ldc; p.ldbias = a.ldbias;
  p.b_gs = a.b_gs; p.c_gs = a.c_gs;
  const int64_t ntn = (a.n + BN - 1) / BN;
  const int64_t blocks = a.form == kGroupedTN
      ? a.groups * ((a.m + BM - 1) / BM) * ntn : (int64_t)p.map_tiles * ntn;
  const dim3 grid((unsigned)blocks), block(NTHR);
  if (a.form == kGroupedNN && a.bias)
    hipLaunchKernelGGL((grouped_gemm_kernel<kGroupedNN, true>), grid, block, 0, s, p);
  else if (a.form == kGroupedNN)
    hipLaunchKernelGGL((grouped_gemm_kernel<kGroupedNN, false>), grid, block, 0, s, p);
  else if (a.form == kGroupedNT)
    hipLaunchKernelGGL((grouped_gemm_kernel<kGroupedNT, false>), grid, block, 0, s, p);
  else
    hipLaunchKernelGGL((grouped_gemm_kernel<kGroupedTN, false>), grid, block, 0, s, p);
}

}  // namespace pa
