// Landmark rows (ba_landmark.hip.h: k_landmark_setup, k_landmark_cost, k_landmark_ne), written once for the device and for the host
// build that pins it (tests/landmark_hostcheck.cpp): the library's detection row (eval_observation_at, ba_math.h) with the spline point
// replaced by a constant world point X.  No time, hence no alpha / beta / rs and no control-point columns, and no visibility test.
//     r = pi_c(X) - obs            signed, predicted minus observed; J = d r / d (the camera's P parameters), signed as well
// P = 6: rvec, t;  P = 15: fx, fy, cx, cy, rvec, t, k1, k2, p1, p2, k3 -- the slot order of ba_math.h without its three sync slots.
#pragma once
#include "ba_math.h"

namespace mvus {

// One row pair at the decoded camera `cam` (CamState as k_cam_states leaves it).  u_obs / v_obs: the observed pixel under fixed
// calibration (undistorted once at set time); with calib the raw pixel is undistorted here with the unknown K and d when `undist`.
// JAC: emit(axis, i, v) is called once for every one of the 2 x P derivatives (axis 0: u, 1: v; i in the order above).
template <bool JAC, class Emit>
MVUS_HD void landmark_row(const CamState& cam, bool calib, bool undist, const double X[3], double u_raw, double v_raw, double u_obs, double v_obs,
                          double& ru, double& rv, Emit&& emit) {
  const double* R = cam.R;
  const double y0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2];
  const double y1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2];
  const double y2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2];
  const double Xc0 = y0 + cam.t[0], Xc1 = y1 + cam.t[1], Xc2 = y2 + cam.t[2];
  const double iz = 1.0 / Xc2;
  const double xn = Xc0 * iz, yn = Xc1 * iz;
  const double uh = cam.fx * xn + cam.cx;
  const double vh = cam.fy * yn + cam.cy;

  double uo = u_obs, vo = v_obs;
  double oxn = 0.0, oyn = 0.0, ox0 = 0.0, oy0 = 0.0, tdx[7], tdy[7];
  if (calib) {
    if (undist) {
      ox0 = (u_raw - cam.cx) / cam.fx;
      oy0 = (v_raw - cam.cy) / cam.fy;
      undistort5<JAC>(ox0, oy0, cam.d, oxn, oyn, tdx, tdy);
      uo = cam.fx * oxn + cam.cx;
      vo = cam.fy * oyn + cam.cy;
    } else {
      uo = u_raw; vo = v_raw;
    }
  }
  ru = uh - uo; rv = vh - vo;
  if (!JAC) return;

  // d(uh)/dXc, d(vh)/dXc
  const double au0 = cam.fx * iz, au2 = -cam.fx * xn * iz;
  const double av1 = cam.fy * iz, av2 = -cam.fy * yn * iz;
  // rotation vector: d Xc / d r = -[y]x W  ->  row a gives (y x a)^T W
  const double cu0 = y1 * au2, cu1 = y2 * au0 - y0 * au2, cu2 = -y1 * au0;      // y x (au0, 0, au2)
  const double cv0 = y1 * av2 - y2 * av1, cv1 = -y0 * av2, cv2 = y0 * av1;      // y x (0, av1, av2)
  const double* W = cam.W;
  const int o = calib ? 4 : 0;      // first of rvec
  emit(0, o + 0, cu0 * W[0] + cu1 * W[3] + cu2 * W[6]);
  emit(0, o + 1, cu0 * W[1] + cu1 * W[4] + cu2 * W[7]);
  emit(0, o + 2, cu0 * W[2] + cu1 * W[5] + cu2 * W[8]);
  emit(1, o + 0, cv0 * W[0] + cv1 * W[3] + cv2 * W[6]);
  emit(1, o + 1, cv0 * W[1] + cv1 * W[4] + cv2 * W[7]);
  emit(1, o + 2, cv0 * W[2] + cv1 * W[5] + cv2 * W[8]);
  // translation
  emit(0, o + 3, au0); emit(0, o + 4, 0.0); emit(0, o + 5, au2);
  emit(1, o + 3, 0.0); emit(1, o + 4, av1); emit(1, o + 5, av2);
  if (calib) {
    // r_u = fx xn + cx - (fx oxn + cx),  oxn = undist((u_raw - cx) / fx, (v_raw - cy) / fy; d)
    double duo[9], dvo[9];      // d(uo), d(vo) / d(fx, fy, cx, cy, k1, k2, p1, p2, k3)
    if (undist) {
      duo[0] = oxn - ox0 * tdx[0];
      duo[1] = -cam.fx * tdx[1] * oy0 / cam.fy;
      duo[2] = 1.0 - tdx[0];
      duo[3] = -cam.fx * tdx[1] / cam.fy;
      dvo[0] = -cam.fy * tdy[0] * ox0 / cam.fx;
      dvo[1] = oyn - oy0 * tdy[1];
      dvo[2] = -cam.fy * tdy[0] / cam.fx;
      dvo[3] = 1.0 - tdy[1];
      for (int k = 0; k < 5; ++k) { duo[4 + k] = cam.fx * tdx[2 + k]; dvo[4 + k] = cam.fy * tdy[2 + k]; }
    } else {
      for (int k = 0; k < 9; ++k) { duo[k] = 0.0; dvo[k] = 0.0; }
    }
    emit(0, 0, xn - duo[0]); emit(0, 1, -duo[1]); emit(0, 2, 1.0 - duo[2]); emit(0, 3, -duo[3]);
    emit(1, 0, -dvo[0]); emit(1, 1, yn - dvo[1]); emit(1, 2, -dvo[2]); emit(1, 3, 1.0 - dvo[3]);
    for (int k = 0; k < 5; ++k) { emit(0, 10 + k, -duo[4 + k]); emit(1, 10 + k, -dvo[4 + k]); }
  }
}

// The observed pixel of a landmark observation under FIXED calibration with undist_points, computed once at set time: what
// k_undistort_fixed does to a detection at create time.
MVUS_HD void landmark_undistort_fixed(const double* Kfix, const double* dfix, int c, double u_raw, double v_raw, double& uo, double& vo) {
  const double fx = Kfix[4 * c], fy = Kfix[4 * c + 1], cx = Kfix[4 * c + 2], cy = Kfix[4 * c + 3];
  double xn, yn;
  undistort5<false>((u_raw - cx) / fx, (v_raw - cy) / fy, dfix + 5 * c, xn, yn, nullptr, nullptr);
  uo = fx * xn + cx;
  vo = fy * yn + cy;
}

// Phase two of k_landmark_ne: entry e = 0 .. P (P + 3) / 2 - 1 is the pair (a, b), a <= b, of the row's augmented vector
// [J_0 .. J_{P-1}, r]: b < P an entry of the triangle of J^T J, b == P the gradient entry J_a^T r.
MVUS_HD int landmark_entries(int P) { return P * (P + 3) / 2; }
MVUS_HD void landmark_entry(int P, int e, int& a, int& b) {
  a = 0;
  while (e >= P + 1 - a) { e -= P + 1 - a; ++a; }
  b = a + e;
}

}  // namespace mvus
