// bf16 transpose [R, C] (row stride ld) -> contiguous [C, R], optionally with
// the fp32 column sums of the input (= row sums of the output: the bias
// gradient when the input is dy).  Feeds the weight gradient a K-contiguous
// operand, docs/KERNELS.md "Wgrad in a K-contiguous layout".
//
// A 256-thread block owns 128 columns and walks a run of 128-row tiles.
// Thread (cg = tid % 16, rg = tid / 16) loads the 8x8 patch at rows rg*8..,
// columns cg*8.. with eight 16-byte loads (16 lanes cover 256 contiguous
// bytes of a row), transposes it in registers, and parks the eight 16-byte
// column pieces in LDS.  The LDS image is the output tile, [128 columns][16
// pieces of 8 rows]; piece p of column c sits in slot p ^ (c / 8 % 16), so
// the 16 lanes of a store (same rg, same k, cg = 0..15) and the 16 lanes of a
// load (same column, p = 0..15) each touch 16 different 16-byte slots.  After
// the barrier thread (p = tid % 16, c = i*16 + tid / 16) reads piece p of
// column c and writes it to out with one 16-byte store, 256 contiguous bytes
// per 16 lanes.  Tiles past R or C load zeros and store nothing.
//
// Column sums: a thread adds its patch rows in row order into 8 fp32
// accumulators kept over the block's row tiles; the 16 row groups meet in LDS
// and are added in rg order; the block writes its chunk's sums to
// ws[chunk][C] with plain stores and ws_reduce adds the chunks in a fixed
// order.  No atomics: two calls give the same bits.
#include "row_io.h"

namespace pa {

namespace {

constexpr int kTile = 128;

struct Patch { uint32_t w[8][4]; };   // 8 rows (or columns) of 8 bf16

__device__ __forceinline__ void load_patch(Patch& p, const short* __restrict__ x,
                                           int64_t row, int64_t col, int64_t ld,
                                           bool ok) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    intx4 v = {0, 0, 0, 0};
    if (ok) v = *reinterpret_cast<const intx4*>(x + (row + j) * ld + col);
#pragma unroll
    for (int q = 0; q < 4; ++q) p.w[j][q] = (uint32_t)v[q];
  }
}

template <bool SUMS>
__global__ __launch_bounds__(256) void transpose_kernel(
    const short* __restrict__ x, short* __restrict__ out, float* __restrict__ ws,
    int R, int C, int64_t ld, int tiles_per_chunk) {
  __shared__ intx4 tile[kTile * 16];   // 32 KB
  const int tid = threadIdx.x, cg = tid & 15, rg = tid >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * kTile;
  const int64_t col = c0 + cg * 8;
  const bool cok = col < C;
  const int nrt = (R + kTile - 1) / kTile;
  const int t0 = blockIdx.y * tiles_per_chunk;
  const int t1 = min(nrt, t0 + tiles_per_chunk);

  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  Patch cur, nxt;
  {
    const int64_t row = (int64_t)t0 * kTile + rg * 8;
    load_patch(cur, x, row, col, ld, cok && t0 < t1 && row < R);
  }
  for (int t = t0; t < t1; ++t) {
    {
      const int64_t row = (int64_t)(t + 1) * kTile + rg * 8;
      load_patch(nxt, x, row, col, ld, cok && t + 1 < t1 && row < R);
    }
    if (SUMS) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[2 * q] += bf2f((short)(cur.w[j][q] & 0xffffu));
          acc[2 * q + 1] += bf2f((short)(cur.w[j][q] >> 16));
        }
    }
    // 8x8 transpose in registers: word m of column k holds rows 2m, 2m+1
    Patch tr;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t a = cur.w[2 * m][q], b = cur.w[2 * m + 1][q];
        tr.w[2 * q][m] = (a & 0xffffu) | (b << 16);
        tr.w[2 * q + 1][m] = (a >> 16) | (b & 0xffff0000u);
      }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      intx4 v = {(int)tr.w[k][0], (int)tr.w[k][1], (int)tr.w[k][2], (int)tr.w[k][3]};
      tile[(cg * 8 + k) * 16 + (rg ^ cg)] = v;
    }
    __syncthreads();
    const int64_t orow = (int64_t)t * kTile + cg * 8;   // here cg is the piece
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = i * 16 + rg;
      const intx4 v = tile[c * 16 + (cg ^ ((c >> 3) & 15))];
      if (c0 + c < C && orow < R)
        *reinterpret_cast<intx4*>(out + (c0 + c) * (int64_t)R + orow) = v;
    }
    __syncthreads();
    cur = nxt;
  }

  if (SUMS) {
    float* red = reinterpret_cast<float*>(tile);   // [16 row groups][128]
    VIO<kF32>::store8(red, rg * kTile + cg * 8, acc);
    __syncthreads();
    if (tid < kTile && c0 + tid < C) {
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) s += red[g * kTile + tid];
      ws[(int64_t)blockIdx.y * C + c0 + tid] = s;
    }
  }
}

}  // namespace

// row chunks: about 2048 blocks in flight, every chunk at least one row tile
TransposePlan transpose_plan(int64_t r, int64_t c) {
  const int64_t xblocks = (c + kTile - 1) / kTile;
  const int64_t nrt = (r + kTile - 1) / kTile;
  const int64_t want = hmin<int64_t>(nrt, hmax<int64_t>(1, 2048 / xblocks));
  TransposePlan p;
  p.tiles_per_chunk = (int)((nrt + want - 1) / want);
  p.chunks = (int)((nrt + p.tiles_per_chunk - 1) / p.tiles_per_chunk);
  return p;
}

void transpose_colsum(const void* x, void* out, float* sums, float* ws,
                      int64_t r, int64_t c, int64_t ld, hipStream_t s) {
  const TransposePlan p = transpose_plan(r, c);
  dim3 grid((unsigned)((c + kTile - 1) / kTile), (unsigned)p.chunks);
  by_flag(sums != nullptr, [&](auto SUMS) {
    hipLaunchKernelGGL((transpose_kernel<SUMS()>), grid, dim3(256), 0, s,
                       (const short*)x, (short*)out, ws, (int)r, (int)c, ld,
                       p.tiles_per_chunk);
  });
  if (sums) ws_reduce(ws, sums, nullptr, p.chunks, 1, c, s);
}

}  // namespace pa
