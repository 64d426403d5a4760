// TEST-ONLY host build of the row routines of the per-detection covariance (mvus_amd/csrc/ba_detcov_math.h): the same source k_detcov
// compiles, behind a C face for ctypes (tests/detcov_hostcheck_util.py).  Built with -ffp-contract=off: the sums are the ones written.
#include "../mvus_amd/csrc/ba_detcov_math.h"

using namespace mvus;

extern "C" {

// Pi = (uu, uv, vv) and the three terms of the split for B = 9 or 18 camera slots; returns 0, or -1 for another B
int detcheck_row(int B, const double* ax, const double* ay, const double* bx, const double* by, const double* Scc, long long lds,
                 const double* T, long long ldt, const double* bp, double* pi, double* terms) {
  if (B == 9) detcov_row<9>(ax, ay, bx, by, Scc, lds, T, ldt, bp, pi, terms);
  else if (B == 18) detcov_row<18>(ax, ay, bx, by, Scc, lds, T, ldt, bp, pi, terms);
  else return -1;
  return 0;
}

void detcheck_image_axes(const double* pi, double su, double sv, double* p) { detcov_image_axes(pi, su, sv, p); }

double detcheck_t2(const double* pi, double sigma2, double ru, double rv) { return detcov_t2(pi, sigma2, ru, rv); }

}
