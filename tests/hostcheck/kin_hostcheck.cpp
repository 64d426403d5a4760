// TEST-ONLY host build of the kinematics routines (mvus_amd/csrc/spline_kin_math.h): what the kernels k_spline_eval_der,
// k_spline_kin_cov_eval and k_span_length / k_span_prefix / k_spline_length of spline_ops.hip.h run per lane, in sequence here so that
// tests/test_kinematics_host.py can pin the arithmetic without a GPU.
#include <cmath>

#include "../../mvus_amd/csrc/spline_kin_math.h"

using namespace mvus;

extern "C" {

// basis of the span whose knot window is tt[6]: the new routine, and bspline_basis_w<true> beside it
void kincheck_basis(const double* tt, double x, double* h, double* dh, double* ddh) { bspline_basis_d2_w(tt, x, h, dh, ddh); }
void kincheck_basis_ref(const double* tt, double x, double* h, double* dh) { bspline_basis_w<true>(tt, x, h, dh); }

// k_spline_eval_der for one spline: t[n + 4] knots, c = cx(n) cy(n) cz(n), D[(nder + 1)][3][nt]
void kincheck_eval_der(const double* t, int n, const double* c, long long nt, const double* x, int nder, double* D) {
  for (long long i = 0; i < nt; ++i) {
    const int l = find_span(t, n, x[i]);
    double H[3][4];
    bspline_basis_d2(t, l, x[i], H[0], H[1], H[2]);
    for (int v = 0; v <= nder; ++v)
      for (int d = 0; d < 3; ++d) {
        double o = 0.0;
        for (int q = 0; q < 4; ++q) o = o + c[d * n + l - 3 + q] * H[v][q];
        D[(3 * v + d) * nt + i] = o;
      }
  }
}

// the state covariance of one sample: H[12] = h, dh, ddh; bp = &band[p][0][0][0]; out[D * D], D = 3 (nder + 1)
void kincheck_state_cov(int nder, const double* H, const double* bp, double* out) {
  if (nder == 0) kin_state_cov<0>(H, bp, out);
  else if (nder == 1) kin_state_cov<1>(H, bp, out);
  else kin_state_cov<2>(H, bp, out);
}

double kincheck_speed_std(const double* v, const double* C, int ld) { return kin_speed_std(v, C, ld); }

// mvus_spline_length for one spline on [lo, hi]: dist[nt] and the interval's length, the three steps in the kernels' order
double kincheck_path_length(const double* t, int n, const double* c, double lo, double hi, long long nt, const double* x, double* dist) {
  double total = 0.0;
  for (int l = 3; l < n; ++l) total = total + kin_span_part(t, n, c, l, lo, hi, hi);
  for (long long i = 0; i < nt; ++i) {
    const int li = find_span(t, n, x[i]);
    double prefix = 0.0;
    for (int l = 3; l < li; ++l) prefix = prefix + kin_span_part(t, n, c, l, lo, hi, hi);
    dist[i] = prefix + kin_span_part(t, n, c, li, lo, hi, x[i]);
  }
  return total;
}

}  // extern "C"
