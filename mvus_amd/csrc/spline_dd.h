// Double-double arithmetic of the spline fit, and the scalar operations its solvers are written in for both precisions
// (T = double or dd).  Host and device.
#pragma once
#include <cmath>

#include "ba_math.h"      // MVUS_HD

namespace mvus {

// Double-double arithmetic (~32 digits) for the passes whose normal equations are too ill conditioned for fp64: a knot set
// with almost as many knots as samples can push cond(A) to 1e10 (cond(A^T A) = 1e20); FITPACK's Givens rotations work on A
// itself.  Products of doubles are exact (FMA), sums carry their rounding error.
// The error-free transformations below are only error free when every operation rounds on its own: no fusing of a product
// with a neighbouring sum (hipcc contracts by default).
#if defined(__clang__)
#define MVUS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MVUS_NO_CONTRACT
#endif
struct dd {
  double hi, lo;
  dd() = default;
  MVUS_HD dd(double h) : hi(h), lo(0.0) {}
  MVUS_HD dd(double h, double l) : hi(h), lo(l) {}
};
MVUS_HD dd dd_quick(double a, double b) { MVUS_NO_CONTRACT const double s = a + b; return dd(s, b - (s - a)); }
MVUS_HD dd dd_two_sum(double a, double b) { MVUS_NO_CONTRACT const double s = a + b, bb = s - a; return dd(s, (a - (s - bb)) + (b - bb)); }
MVUS_HD dd dd_two_prod(double a, double b) { MVUS_NO_CONTRACT const double p = a * b; return dd(p, fma(a, b, -p)); }
MVUS_HD dd operator+(dd a, dd b) { MVUS_NO_CONTRACT dd s = dd_two_sum(a.hi, b.hi); s.lo += a.lo + b.lo; return dd_quick(s.hi, s.lo); }
MVUS_HD dd operator-(dd a) { return dd(-a.hi, -a.lo); }
MVUS_HD dd operator-(dd a, dd b) { return a + (-b); }
MVUS_HD dd operator*(dd a, dd b) { MVUS_NO_CONTRACT dd p = dd_two_prod(a.hi, b.hi); p.lo += a.hi * b.lo + a.lo * b.hi; return dd_quick(p.hi, p.lo); }
MVUS_HD dd operator/(dd a, dd b) {
  MVUS_NO_CONTRACT
  const double q1 = a.hi / b.hi;
  dd r = a - b * dd(q1);
  const double q2 = r.hi / b.hi;
  r = r - b * dd(q2);
  const double q3 = r.hi / b.hi;
  return dd_quick(q1, q2) + dd(q3);
}
MVUS_HD dd& operator+=(dd& a, dd b) { a = a + b; return a; }
MVUS_HD dd& operator-=(dd& a, dd b) { a = a - b; return a; }
MVUS_HD dd& operator/=(dd& a, dd b) { a = a / b; return a; }
MVUS_HD dd num_sqrt(dd a) {                        // Karp / Markstein: one correction of the fp64 square root
  MVUS_NO_CONTRACT
  const double x = 1.0 / sqrt(a.hi), ax = a.hi * x;
  const dd r = a - dd_two_prod(ax, ax);
  return dd_two_sum(ax, r.hi * (x * 0.5));
}
MVUS_HD double num_sqrt(double a) { return sqrt(a); }
MVUS_HD double to_double(double a) { return a; }
MVUS_HD double to_double(dd a) { return a.hi + a.lo; }
MVUS_HD bool is_positive(double a) { return a > 0.0; }
MVUS_HD bool is_positive(dd a) { return a.hi > 0.0; }
MVUS_HD double pivot_floor(double) { return 1e-12; }       // a Cholesky pivot below this fraction of its diagonal entry is lost to rounding
MVUS_HD double pivot_floor(dd) { return 1e-24; }
MVUS_HD double num_prod(double a, double b, double) { return a * b; }          // a * b in the precision of the third argument
MVUS_HD dd num_prod(double a, double b, dd) { return dd_two_prod(a, b); }

MVUS_HD double num_recip(double a) { return 1.0 / a; }
MVUS_HD dd num_recip(dd a) {                        // one Newton step on the fp64 reciprocal: r0 + r0 (1 - a r0)
  MVUS_NO_CONTRACT
  const double r0 = 1.0 / a.hi;
  dd p = dd_two_prod(a.hi, r0);
  p.lo += a.lo * r0;
  const dd e = dd(1.0) - dd_quick(p.hi, p.lo);
  return dd_two_sum(r0, r0 * (e.hi + e.lo));
}

}  // namespace mvus
