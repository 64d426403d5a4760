// Position priors on the trajectory (ba_prior.hip.h: k_prior_setup, k_prior_cost, k_prior_ne), written once for the device and for the
// host build that pins it (tests/priors_hostcheck.cpp): where a prior's time falls on the splines, the four cubic B-spline weights of
// its knot span, and its three residual rows at x.  Plain C++, no device intrinsics.
#pragma once
#include "ba_math.h"

namespace mvus {

// The interval [start, end] that holds t, BOTH ends closed (a prior at the last instant of a flight is a prior like any other; the
// detection rows keep util.py:105's half-open rule), or -1.  Intervals are sorted and disjoint (HostProblem::build checks it).
MVUS_HD int prior_interval(const double* istart, const double* iend, int S, double t) {
  int lo = 0, hi = S;  // last interval whose start <= t
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t >= istart[mid]) lo = mid; else hi = mid;
  }
  return (t >= istart[lo] && t <= iend[lo]) ? lo : -1;
}

// One prior at set time: the global index of the first of its four control points (-1: t lies in no interval, the prior is inactive and
// h is zero) and the weights h_a(t) on control points ctrl .. ctrl + 3.  The span is FITPACK's (find_span: t[l] <= t < t[l+1], the last
// span at t = end, so the weights there are the right-end values splev gives) and the weights are fpbspl's recurrence as the detection
// rows run it (bspline_basis_w).  Neither depends on x.
MVUS_HD int32_t prior_setup_row(const SplineView& sp, double t, double h[4]) {
  h[0] = h[1] = h[2] = h[3] = 0.0;
  const int s = prior_interval(sp.istart, sp.iend, sp.S, t);
  if (s < 0) return -1;
  const double* kn = sp.knots + sp.knot_off[s];
  const int n = sp.ctrl_off[s + 1] - sp.ctrl_off[s];
  const int l = find_span(kn, n, t);
  double dh[4];
  bspline_basis<false>(kn, l, t, h, dh);
  return sp.ctrl_off[s] + (l - 3);
}

// S(t) - p of one active prior: x0[a] = index in x of the x coordinate of control point ctrl + a, stride[a] the distance to its y and z
// (MotionView::ctrl_x0 / ctrl_stride).  The sum runs over the four control points in their order: k_prior_cost and k_prior_ne read the
// same bits.
MVUS_HD void prior_diff(const double* x, const int32_t x0[4], const int32_t stride[4], const double h[4], const double p[3], double diff[3]) {
  for (int d = 0; d < 3; ++d) {
    double s = 0.0;
    for (int a = 0; a < 4; ++a) s = s + h[a] * x[x0[a] + d * stride[a]];
    diff[d] = s - p[d];
  }
}

}  // namespace mvus
