// TEST-ONLY host build of the landmark row routine (mvus_amd/csrc/ba_landmark_math.h): what k_landmark_cost and phase one of
// k_landmark_ne evaluate per row, and the entry map of phase two, so that tests/test_landmarks_host.py can pin the arithmetic without
// a GPU.
#include "../mvus_amd/csrc/ba_landmark_math.h"

using namespace mvus;

extern "C" {

// one observation: params[P] in x's order (P = 15 under calib, else 6; K4 / d5 the fixed calibration then), r[2] and J[2 * P] out,
// weighted as the kernels weight them
void landmarkcheck_row(int calib, int undist, const double* K4, const double* d5, const double* params, const double* X, const double* uv,
                       const double* w, double* r, double* J) {
  const int P = calib ? 15 : 6;
  CamState cam{};
  const double* rv;
  if (calib) {
    cam.fx = params[0]; cam.fy = params[1]; cam.cx = params[2]; cam.cy = params[3];
    rv = params + 4;
    for (int k = 0; k < 3; ++k) cam.t[k] = params[7 + k];
    for (int k = 0; k < 5; ++k) cam.d[k] = params[10 + k];
  } else {
    cam.fx = K4[0]; cam.fy = K4[1]; cam.cx = K4[2]; cam.cy = K4[3];
    rv = params;
    for (int k = 0; k < 3; ++k) cam.t[k] = params[3 + k];
    for (int k = 0; k < 5; ++k) cam.d[k] = d5[k];
  }
  rodrigues(rv, cam.R, cam.W);
  double uo = uv[0], vo = uv[1];
  if (!calib && undist) landmark_undistort_fixed(K4, d5, 0, uv[0], uv[1], uo, vo);
  double ru, rvv;
  landmark_row<true>(cam, calib != 0, undist != 0, X, uv[0], uv[1], uo, vo, ru, rvv,
                     [&](int axis, int i, double v) { J[axis * P + i] = w[axis] > 0.0 ? w[axis] * v : 0.0; });
  r[0] = w[0] > 0.0 ? w[0] * ru : 0.0;
  r[1] = w[1] > 0.0 ? w[1] * rvv : 0.0;
}

int landmarkcheck_entries(int P) { return landmark_entries(P); }
void landmarkcheck_entry(int P, int e, int* a, int* b) { landmark_entry(P, e, *a, *b); }

}  // extern "C"
