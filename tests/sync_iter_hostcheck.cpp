// TEST-ONLY host build of the lane routines of the iterative time-shift search (mvus_amd/csrc/sync_iter_math.h), compiled with g++ by
// tests/sync_iter_hostcheck_util.py.  Not part of the product.
#include <cstdint>
#include <vector>

#include "../mvus_amd/csrc/sync_iter_math.h"

using namespace mvus;

extern "C" {

void sicheck_sample9(uint64_t seed, int round, int sign, int h, long long n, long long* idx) { si_sample9(seed, round, sign, h, n, idx); }

int sicheck_betas(const double* s1, const double* s2, const double* ds, double* betas) {
  std::vector<double> w(kSiPencilWork);
  return si_pencil_betas(s1, s2, ds, w.data(), 1, betas);
}

// real eigenvalues of a 6 x 6 matrix (row-major, left untouched): their number, -1 without convergence
int sicheck_eig6(const double* a, double* wr) {
  double c[36];
  for (int i = 0; i < 36; ++i) c[i] = a[i];
  return si_real_eig6(c, 1, wr);
}

int sicheck_fundamental(const double* x1, const double* x2, double* F) {
  std::vector<double> w(kSiFitWork);
  return si_fundamental9(x1, x2, w.data(), 1, F) ? 1 : 0;
}

void sicheck_spline(const double* t, const double* c, int n, long long m, const double* u, double* out) {
  for (long long i = 0; i < m; ++i) {
    double o[2];
    si_spline_eval2(t, c, n, u[i], o);
    out[i] = o[0]; out[m + i] = o[1];
  }
}

int sicheck_span(const double* t, int n, double u, int guess) { return guess ? si_find_span_guess(t, n, u) : find_span(t, n, u); }

double sicheck_sampson(const double* F, double u1, double v1, double u2, double v2) { return si_sampson(F, u1, v1, u2, v2); }

int sicheck_in_intervals(const double* iv, int K, double tau) { return si_in_intervals(iv, K, tau) ? 1 : 0; }

}  // extern "C"
