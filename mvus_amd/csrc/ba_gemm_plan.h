// Tiles and K-slabs of the Schur product (k_schur_gemm in ba_schur_product.hip.h): which workgroup computes which 48x48 tile, where the
// nine 16x16 accumulators of a tile go, and how many K-slabs the product is cut into.  Plain C++ (no HIP), shared by the kernel, its
// host side and a stand-alone host check (tests/hostcheck/gemm_plan_hostcheck.cpp).
#pragma once
#include <algorithm>

#if defined(__HIPCC__)
#define MVUS_GEMM_HD __host__ __device__ inline
#else
#define MVUS_GEMM_HD inline
#endif

namespace mvus {

constexpr int kGemmT = 48;
constexpr int kGemmUn = 4;                                 // k-steps (of 4 rows) per operand set
constexpr int kGemmSetRows = 4 * kGemmUn;

// 48-wide block rows of the CB x CB product, and its tiles: the block lower triangle, diagonal included.  The right-hand-side column
// (column CB) has no tiles of its own: it rides in the diagonal tiles (gemm_sub).
MVUS_GEMM_HD int gemm_blocks(int CB) { return (CB + kGemmT - 1) / kGemmT; }
MVUS_GEMM_HD int gemm_tiles(int CB) { const int nbk = gemm_blocks(CB); return nbk * (nbk + 1) / 2; }

// tile t of the block lower triangle, row by row: t = bi (bi + 1) / 2 + bj, bj <= bi
MVUS_GEMM_HD void gemm_tile_decode(int t, int& bi, int& bj) {
  bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;             // (at most 24 steps: CB <= 1152)
  bj = t - bi * (bi + 1) / 2;
}

// Accumulator (i, j) of a tile, i, j in 0..2.  Off the diagonal it is the 16x16 sub-block (i, j) of the tile.  On the diagonal only
// j <= i is: the product is symmetric and its readers take (j, i) for (i, j), so the three accumulators above the diagonal carry
// the right-hand-side column instead -- (0,1), (0,2), (1,2) hold rows 0-15, 16-31, 32-47 of the tile's block row times column CB
// of the second operand (all sixteen columns of the fragment alike; column 0 is stored).
struct GemmSub { int rb, cb; bool rhs; };                   // 16-row piece rb of the block row; 16-column piece cb of the block column, or the rhs column
MVUS_GEMM_HD GemmSub gemm_sub(bool diag, int i, int j) {
  if (diag && j > i) return GemmSub{i + j - 1, 0, true};
  return GemmSub{i, j, false};
}

// K-slabs of the Schur product: a slab's tiles run on one XCD, two workgroups per CU, so the time is (rounds of the busiest XCD's
// slots) x (row sets per wavefront); the slab count with the least of that (ties: fewer slabs = fewer partial sums for the reduced
// system's first kernel).  rows: the product's main K range; cus: compute units of the device (eight XCDs); forced > 0: that count.
inline int gemm_plan_slabs(int CB, int rows, int cus, int forced) {
  if (forced > 0) return forced;
  const int tiles = gemm_tiles(CB);
  const int slots = std::max(8, 2 * cus), nsets = std::max(1, (rows + kGemmSetRows - 1) / kGemmSetRows);
  int nslab = 1;
  double best = 1e300;
  for (int s = 1; s <= 128 && 4 * s <= nsets; ++s) {
    const int per_wave = (nsets + 4 * s - 1) / (4 * s);                       // sets of the busiest wavefront
    const int on_xcd = tiles * ((s + 7) / 8);                                 // workgroups of the busiest XCD
    const double cost = (double)((on_xcd + slots / 8 - 1) / (slots / 8)) * (per_wave + 1.5) + 0.002 * s;
    if (cost < best * 0.995) { best = cost; nslab = s; }
  }
  return nslab;
}
// workgroups the launch puts on the busiest XCD (workgroup L runs on XCD L % 8; slab s on XCD s % 8)
inline int gemm_xcd_load(int CB, int nslab) { return gemm_tiles(CB) * ((nslab + 7) / 8); }
// grid of k_schur_gemm
inline unsigned gemm_grid(int CB, int nslab) { return 8u * (unsigned)gemm_tiles(CB) * (unsigned)((nslab + 7) / 8); }

}  // namespace mvus
