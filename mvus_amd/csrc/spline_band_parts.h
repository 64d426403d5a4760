// The partition of a banded system into interiors and separators (k_band_solve_parts): the arithmetic of who owns which row.
// Host and device; the host tests build it with g++.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "ba_math.h"      // MVUS_HD

namespace mvus {

struct BandParts {
  int P = 1, len = 0, rem = 0, HB = 3;       // interior p: rows [first(p), first(p) + length(p)), then HB separator rows
  MVUS_HD int length(int p) const { return len + (p < rem ? 1 : 0); }
  MVUS_HD int first(int p) const { return p * (len + HB) + (p < rem ? p : rem); }
  // row j -> its interior p and the row i inside it (i >= length(p): a separator row)
  MVUS_HD void locate(int j, int& p, int& i) const {
    const int big = len + 1 + HB;
    if (j < rem * big) { p = j / big; i = j - p * big; }
    else { const int j2 = j - rem * big; p = rem + j2 / (len + HB); i = j2 - (p - rem) * (len + HB); }
  }
  // the interiors' rows are also kept TRANSPOSED for the solver: value k of K per row, row i of interior p at ((i K + k) P + p),
  // so that the P lanes of k_band_solve_parts (one interior each) read and write consecutive addresses
  MVUS_HD long long at(int p, int i, int k, int K) const { return ((long long)i * K + k) * P + p; }
};
constexpr int kBandPartsMax = 256;
// n rows can be cut into P interiors: one lane each (P <= kBandPartsMax), every interior at least 2 HB rows long
inline bool band_parts_legal(int n, int HB, int P) { return P >= 2 && P <= kBandPartsMax && n > (P - 1) * HB && (n - (P - 1) * HB) / P >= 2 * HB; }
// exactly P interiors (a legal P): the first rem of them have len + 1 rows, the others len
inline BandParts band_parts_fixed(int n, int HB, int P) {
  BandParts bp;
  bp.HB = HB;
  bp.P = P;
  bp.len = (n - (P - 1) * HB) / P;
  bp.rem = (n - (P - 1) * HB) - bp.len * P;
  return bp;
}
// the production rule: one chain below min_rows, else about sqrt(n / 2.5) interiors of at least 2 HB rows
inline BandParts band_parts(int n, int HB, int min_rows) {
  BandParts bp;
  bp.HB = HB;
  if (n < min_rows) return bp;
  static const double scale = [] { const char* e = std::getenv("MVUS_BAND_PARTS_SCALE"); return e ? std::atof(e) : 1.0; }();      // (experiments)
  int P = (int)(scale * std::sqrt((double)n / 2.5));
  P = std::max(2, std::min(kBandPartsMax, P));
  while (P > 1 && (n - (P - 1) * HB) / P < 2 * HB) --P;
  if (P < 2) return bp;
  return band_parts_fixed(n, HB, P);
}

}  // namespace mvus
