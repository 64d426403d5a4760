// TEST-ONLY stand-alone host program around mvus_amd/csrc/ba_gemm_plan.h: the tile decode and the accumulator map of k_schur_gemm, and
// the slab plan.  Built and run by tests/test_gemm_plan_host.py (g++, no HIP).
//   gemm_plan_hostcheck cover                      every tile once, every needed 16x16 sub-block and rhs piece written once; "ok" or a message + exit 1
//   gemm_plan_hostcheck plan CB rows cus forced    prints "nslab xcd_load grid"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string_view>
#include <utility>

#include "../../mvus_amd/csrc/ba_gemm_plan.h"

using namespace mvus;

static int fail(const char* what, int CB, int x, int y) {
  std::printf("CB = %d: %s (%d, %d)\n", CB, what, x, y);
  return 1;
}

// the stores of k_schur_gemm's epilogue at 16x16 granularity, for one slab of a CB-column product
static int cover(int CB) {
  const int nbk = gemm_blocks(CB), tiles = gemm_tiles(CB), n16 = (CB + 15) / 16;
  if (tiles != nbk * (nbk + 1) / 2) return fail("tile count", CB, tiles, nbk);
  std::set<std::pair<int, int>> seen;
  std::map<std::pair<int, int>, int> sub;        // (16-row piece, 16-column piece) -> writers
  std::map<int, int> rhs;                        // 16-row piece of column CB -> writers
  for (int t = 0; t < tiles; ++t) {
    int bi = -1, bj = -1;
    gemm_tile_decode(t, bi, bj);
    if (bi < 0 || bi >= nbk || bj < 0 || bj > bi) return fail("tile outside the block lower triangle", CB, bi, bj);
    if (!seen.insert({bi, bj}).second) return fail("tile produced twice", CB, bi, bj);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const GemmSub s = gemm_sub(bi == bj, i, j);
        if (s.rb < 0 || s.rb > 2 || s.cb < 0 || s.cb > 2) return fail("piece outside the tile", CB, s.rb, s.cb);
        const int R = 3 * bi + s.rb, Cc = 3 * bj + s.cb;
        if (R >= n16) continue;                  // rows beyond the matrix: the epilogue stores nothing
        if (s.rhs) ++rhs[R];
        else if (Cc < n16) {
          if (Cc > R) return fail("sub-block above the diagonal written", CB, R, Cc);
          ++sub[{R, Cc}];
        }
      }
  }
  if ((int)seen.size() != tiles) return fail("tiles missing", CB, (int)seen.size(), tiles);
  for (int R = 0; R < n16; ++R) {
    for (int Cc = 0; Cc <= R; ++Cc)
      if (sub[{R, Cc}] != 1) return fail("sub-block not written exactly once", CB, R, Cc);
    if (rhs[R] != 1) return fail("rhs piece not written exactly once", CB, R, rhs[R]);
  }
  // what the readers take for entry (a, b): (hi, lo) at 16-column granularity -- always a sub-block on or below the diagonal
  for (int a = 0; a < CB; a += 5)
    for (int b = 0; b < CB; b += 7) {
      const int hi = a / 16 >= b / 16 ? a : b, lo = a / 16 >= b / 16 ? b : a;
      if (sub.find({hi / 16, lo / 16}) == sub.end()) return fail("reader takes an unwritten sub-block", CB, a, b);
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string_view(argv[1]) == "cover") {
    for (int nbk = 1; nbk <= 24; ++nbk)
      for (int CB : {48 * nbk, 48 * (nbk - 1) + 1, 48 * (nbk - 1) + 9, 48 * (nbk - 1) + 16, 48 * (nbk - 1) + 17, 48 * (nbk - 1) + 33}) {
        if (gemm_blocks(CB) != nbk) return fail("block count", CB, gemm_blocks(CB), nbk);
        if (cover(CB)) return 1;
      }
    std::printf("ok\n");
    return 0;
  }
  if (argc == 6 && std::string_view(argv[1]) == "plan") {
    const int CB = std::atoi(argv[2]), rows = std::atoi(argv[3]), cus = std::atoi(argv[4]), forced = std::atoi(argv[5]);
    const int nslab = gemm_plan_slabs(CB, rows, cus, forced);
    std::printf("%d %d %u\n", nslab, gemm_xcd_load(CB, nslab), gemm_grid(CB, nslab));
    return 0;
  }
  std::fprintf(stderr, "usage: %s cover | plan CB rows cus forced\n", argv[0]);
  return 2;
}
