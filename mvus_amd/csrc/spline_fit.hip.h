// Smoothing-spline fit of a 3-D trajectory on the GPU: Scene.traj_to_spline's scipy.interpolate.splprep(X, u=t, s=s, k=3)
// (reference common.py:247, 267), i.e. FITPACK parcur / fppara (Dierckx) with iopt = 0, nest = m + 2k; unit weights as the reference
// calls it, or splprep's w (one positive scalar per sample) in the _w kernels: the two places where fppara reads w.
//
// Same algorithm, different linear algebra.  fppara's control flow runs on the host (fit_smoothing_spline below: knots are
// added where the residual of the least-squares spline is largest until f(p = inf) <= s, then the smoothing parameter p with
// F(p) = s is found by rational interpolation -- fpknot, fprati and fpdisc are restated line by line, they are O(knots) integer
// / scalar work).  Everything that touches the m samples or solves a system runs on the device:
//   k_fit_basis      knot span + the four cubic B-splines of every sample (the fpbspl recurrence of ba_math.h)
//   k_fit_blocks     per knot span: sum of h h^T and h x^T over its samples (fixed-order tree per workgroup); k_fit_blocks_w: of (w h)(w h)^T, (w h)(w x)^T
//   k_fit_band       banded normal equations A^T A (half-bandwidth 3) and A^T X from <= 4 span blocks per entry
//   k_fit_penalty    B^T B of fpdisc's discontinuity-jump matrix (half-bandwidth 4);  k_fit_combine: A^T A + B^T B / p^2 (fppara rotates the rows of B in with weight 1/p)
//   k_band_solve     banded Cholesky + both substitutions, one wavefront, the previous rows in registers; in fp64, and again in
//                    double-double when a pivot is lost to rounding (knot sets close to interpolation: cond(A) ~ 1e10)
//   k_fit_residual   per-sample squared residual (k_fit_residual_w: of w (s(u) - x));  k_fit_fpint: per-span sums with FITPACK's half/half rule for the sample
//                    that sits on a knot, and the total f_p
// FITPACK rotates every observation row (and, in the p iteration, every row of B all the way down the band: O(n^2)) into a
// triangle with Givens rotations, one after the other; the normal equations give the same splines (same knots on every fixture
// and seeded case of tests/test_traj_to_spline.py, coefficients to ~1e-9 relative) in O(m + n) parallel work per pass.

// This header has no code of its own: it names the headers of the fit.
#pragma once
#include "spline_dd.h"                        // the double-double type, scalar operations for T = double or dd
#include "spline_band_parts.h"                // BandParts and the partition rules (host and device)
#include "spline_fit_passes.hip.h"            // size rules; k_fit_basis .. k_fit_combine, k_fit_residual, k_fit_fpint*, k_fit_total*
#include "spline_band_solve.hip.h"            // k_band_solve, k_band_diag_sum
#include "spline_band_solve_parts.hip.h"      // k_band_solve_parts
#include "spline_fit_weighted.hip.h"          // k_fit_blocks_w, k_fit_wx2, k_fit_fp_from_factor, k_fit_residual_w
#include "spline_fitpack_host.h"              // namespace fitpack: fpdisc, fpknot, fpknot_batch, fprati
