// Shared by the dense MFMA GEMM kernels (gemm.hip, gemm_fp8.hip): the
// workgroup -> tile mapping and the host-side interior/edge launch plan.
// Both kernels use a 256 x 256 block tile; the host ABI is pa::GemmArgs
// (api.h), the __global__ parameter lists stay scalar.
//
// The conservative main loop and the epilogue's (row, col) walk are NOT
// shared: as __forceinline__ helpers taking the staging / fragment lambdas
// they changed the generated code of the fast kernels (other loop-counter
// code, ~480 more instructions in the epilogue), and register allocation in
// these bodies follows the exact loop form.  Each file writes them once.
#pragma once
#include "common.h"
#include "api.h"

namespace pa {

constexpr int kGemmTile = 256;   // BM == BN

// Tile origin of this workgroup.  T1: XCD-aware bijective workgroup swizzle
// (contiguous chunks of the linear block index per XCD), then CUTLASS-style
// tile-group rasterization: GM consecutive bm-rows walk bn fastest, so the
// ~32 blocks concurrently resident on one XCD touch few A/B panels and their
// K-tile streams coincide in L2 (vs column-major order, which re-reads the B
// panel from HBM for every bm).  A FAST grid spans only the interior tile
// rectangle, an edge grid every tile.
template <bool FAST>
__device__ __forceinline__ void gemm_tile_origin(int M, int N, int& row0, int& col0) {
  constexpr int BM = kGemmTile, BN = kGemmTile;
  const int nwg = gridDim.x * gridDim.y;
  int orig = blockIdx.y * gridDim.x + blockIdx.x;
  {
    const int nx = 8;
    int q = nwg / nx, rr = nwg % nx;
    int xcd = orig % nx, pos = orig / nx;
    orig = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + pos;
  }
  const int mt = FAST ? (M / BM) : ((M + BM - 1) / BM);
  const int nt = FAST ? (N / BN) : ((N + BN - 1) / BN);
  constexpr int GM = 8;
  int bm, bn;
  {
    int band = orig / (GM * nt);
    int rem = orig - band * (GM * nt);
    int gm_band = mt - band * GM < GM ? mt - band * GM : GM;
    bm = band * GM + rem % gm_band;
    bn = rem / gm_band;
  }
  row0 = bm * BM;
  col0 = bn * BN;
}

// ---------------------------------------------------------------------------
// host: interior/edge plan.  The fast kernel covers the rectangle of full
// 256 x 256 tiles when K is a multiple of the K-step and the layout has a
// fast kernel; the guarded kernel runs over the whole grid and its blocks
// return early where the fast launch already computed (skip_interior).
// ---------------------------------------------------------------------------
struct GemmPlan {
  bool has_fast, has_edge;
  dim3 fast_grid, edge_grid;
};

inline GemmPlan gemm_plan(const GemmArgs& g, int bk, bool fast_kernel) {
  const unsigned mi = (unsigned)(g.m / kGemmTile), ni = (unsigned)(g.n / kGemmTile);
  const unsigned gm = (unsigned)((g.m + kGemmTile - 1) / kGemmTile);
  const unsigned gn = (unsigned)((g.n + kGemmTile - 1) / kGemmTile);
  GemmPlan p;
  p.has_fast = fast_kernel && g.k % bk == 0 && mi > 0 && ni > 0;
  p.has_edge = !p.has_fast || mi < gm || ni < gn;
  p.fast_grid = dim3(mi, ni, (unsigned)g.batch);
  p.edge_grid = dim3(gm, gn, (unsigned)g.batch);
  return p;
}

// issue(kernel, grid, skip_interior) launches one kernel of the pair
template <class Kernel, class Issue>
inline void gemm_launch(const GemmPlan& p, Kernel fast, Kernel edge, Issue issue) {
  if (p.has_fast) issue(fast, p.fast_grid, 0);
  if (p.has_edge) issue(edge, p.edge_grid, p.has_fast ? 1 : 0);
}

}  // namespace pa
