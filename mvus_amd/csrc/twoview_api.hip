// libmvusba.so, two-view geometry and PnP: triangulation, PnP RANSAC, fundamental-matrix RANSAC, optimal correction of matches and
// the pose of an essential matrix (include/mvus_ba.h), with the host halves of the epipolar code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "api_common.h"
#include "triangulate.hip.h"
#include "pnp.hip.h"
#include "epipolar.hip.h"
#include "sync_iter.hip.h"

using namespace mvus;

// ---- iterative time-shift search (sync_iter.hip.h): the session ---------------------------------------------------------------
// `mem` holds what open uploads, `work` the per-round buffers, which grow with the number of models asked for.
struct mvus_sync_iter {
  int device = 0;
  hipStream_t st = nullptr;
  DeviceOwner mem, work;
  SiView v{};
  long long cap_h = 0, cap_m = 0;                // hypotheses (both signs) and models the work buffers hold
  double *samp = nullptr, *betas = nullptr, *models = nullptr, *out = nullptr;
  uint8_t* valid = nullptr;
  int32_t* counts = nullptr;
  long long* idx = nullptr;
  template <class T>
  const T* put(const T* host, size_t count) {
    T* d = mem.device<T>(count);
    if (count) MVUS_HIP(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st));
    return d;
  }
  void reserve(long long hyps, long long nmodels) {
    if (hyps <= cap_h && nmodels <= cap_m) return;
    MVUS_HIP(hipStreamSynchronize(st));
    work.reset();
    cap_h = std::max(hyps, cap_h); cap_m = std::max(nmodels, cap_m);
    samp = work.device<double>((size_t)cap_h * kSiSampDoubles);
    betas = work.device<double>((size_t)cap_h * kSiSlots);
    valid = work.device<uint8_t>((size_t)cap_h * kSiSlots);
    idx = work.device<long long>((size_t)cap_h * kSiSample);
    models = work.device<double>((size_t)cap_m * kSiModel);
    counts = work.device<int32_t>((size_t)cap_m * 2);
    out = work.device<double>(8);
  }
  ~mvus_sync_iter() {
    if (st) { (void)hipStreamSynchronize(st); }
    work.reset(); mem.reset();
    if (st) (void)hipStreamDestroy(st);
  }
};

// ---- two-view geometry (epipolar.hip.h): host halves ------------------------------------------------------------------------
namespace {
// eigen-decomposition of a symmetric n x n matrix (row-major, destroyed) by cyclic Jacobi rotations: w[n] ascending, V columns
void sym_eig_jacobi(int n, double* A, double* w, double* V) {
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) V[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, tot = 0.0;
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { tot += A[i * n + j] * A[i * n + j]; if (i != j) off += A[i * n + j] * A[i * n + j]; }
    if (!(off > 1e-30 * tot)) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (apq == 0.0) continue;
        const double th = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(1.0 + th * th));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
        for (int k = 0; k < n; ++k) {                       // A <- J^T A J
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq; A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk; A[q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq; V[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  std::vector<int> ord(n);
  for (int i = 0; i < n; ++i) ord[i] = i;
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return A[a * n + a] < A[b * n + b]; });
  std::vector<double> Vs((size_t)n * n);
  for (int k = 0; k < n; ++k) { w[k] = A[ord[k] * n + ord[k]]; for (int i = 0; i < n; ++i) Vs[i * n + k] = V[i * n + ord[k]]; }
  std::memcpy(V, Vs.data(), sizeof(double) * n * n);
}

// unit right null vector of a 3x3 matrix M (smallest eigenvector of M^T M); left: of M^T
void null3(const double* M, bool left, double* e) {
  double A[9], w[3], V[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += left ? M[3 * i + k] * M[3 * j + k] : M[3 * k + i] * M[3 * k + j];
      A[3 * i + j] = s;
    }
  sym_eig_jacobi(3, A, w, V);
  for (int i = 0; i < 3; ++i) e[i] = V[3 * i];
}

// unit null vector of a rank-2 3x3 matrix as the largest cross product of two of its rows (right) or columns (left): exact to
// rounding for a rank-2 matrix, where an eigenvector of M^T M carries the error of squaring it
void null3_cross(const double* M, bool left, double* e) {
  auto vec = [&](int k, double* v) { for (int a = 0; a < 3; ++a) v[a] = left ? M[3 * a + k] : M[3 * k + a]; };
  double best = -1.0;
  for (int i = 0; i < 2; ++i)
    for (int j = i + 1; j < 3; ++j) {
      double a[3], b[3], c[3];
      vec(i, a); vec(j, b);
      c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
      const double n = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
      if (n > best) { best = n; for (int k = 0; k < 3; ++k) e[k] = c[k]; }
    }
  const double n = std::sqrt(best);
  if (n > 0.0) for (int k = 0; k < 3; ++k) e[k] /= n;
  else null3(M, left, e);
}

// F (normalised coordinates, from the 8-point normal matrix) -> rank 2: F (I - v v^T) with v the right null vector of F
void rank2(double* F) {
  double v[3];
  null3(F, false, v);
  double Fv[3];
  for (int i = 0; i < 3; ++i) Fv[i] = F[3 * i] * v[0] + F[3 * i + 1] * v[1] + F[3 * i + 2] * v[2];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) F[3 * i + j] -= Fv[i] * v[j];
}

double det3h(const double* A) { return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]); }
void mul3(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// compute_Rt_from_E (epipolar.py:513-539): E = U S Vh; Vh <- -Vh when det(U Vh) < 0; R1 = U W Vh, R2 = U W^T Vh (each times its
// determinant), t = +-U[:, 2]; candidates (R1, t), (R1, -t), (R2, t), (R2, -t) as 3x4 row-major
void essential_candidates(const double* E, double (*P)[12]) {
  double A[9], w[3], V[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { double s = 0.0; for (int k = 0; k < 3; ++k) s += E[3 * k + i] * E[3 * k + j]; A[3 * i + j] = s; }
  sym_eig_jacobi(3, A, w, V);                          // ascending: columns 2, 1 are the two large singular directions
  double v[3][3], u[3][3];
  for (int i = 0; i < 3; ++i) { v[0][i] = V[3 * i + 2]; v[1][i] = V[3 * i + 1]; v[2][i] = V[3 * i]; }
  for (int k = 0; k < 2; ++k) {
    double n = 0.0;
    for (int i = 0; i < 3; ++i) { u[k][i] = E[3 * i] * v[k][0] + E[3 * i + 1] * v[k][1] + E[3 * i + 2] * v[k][2]; }
    if (k == 1) { double d = 0.0; for (int i = 0; i < 3; ++i) d += u[1][i] * u[0][i]; for (int i = 0; i < 3; ++i) u[1][i] -= d * u[0][i]; }
    for (int i = 0; i < 3; ++i) n += u[k][i] * u[k][i];
    n = std::sqrt(n);
    for (int i = 0; i < 3; ++i) u[k][i] /= n;
  }
  u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
  u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
  u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  double U[9], Vh[9];
  for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) { U[3 * i + k] = u[k][i]; Vh[3 * k + i] = v[k][i]; }
  double UV[9];
  mul3(U, Vh, UV);
  if (det3h(UV) < 0.0) for (int a = 0; a < 9; ++a) Vh[a] = -Vh[a];
  const double W[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0}, Wt[9] = {0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  double T[9], R1[9], R2[9];
  mul3(U, W, T); mul3(T, Vh, R1);
  mul3(U, Wt, T); mul3(T, Vh, R2);
  const double d1 = det3h(R1), d2 = det3h(R2);
  for (int a = 0; a < 9; ++a) { R1[a] *= d1; R2[a] *= d2; }
  const double* Rs[4] = {R1, R1, R2, R2};
  for (int c = 0; c < 4; ++c) {
    const double sg = (c & 1) ? -1.0 : 1.0;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) P[c][4 * i + j] = Rs[c][3 * i + j];
      P[c][4 * i + 3] = sg * U[3 * i + 2];
    }
  }
}

int epi_fail(const char* msg, int code) { g_create_error = msg; return code; }
}  // namespace

extern "C" {

int mvus_triangulate(int32_t device, int64_t N, const double* x1, const double* x2, const double* P1, const double* P2,
                     double* X, double* err1, double* err2) {
  if (N < 0 || !P1 || !P2 || (N > 0 && (!x1 || !x2 || !X))) { g_create_error = "triangulate: bad arguments"; return MVUS_E_INVALID; }
  if (N == 0) return MVUS_OK;
  return stateless([&] {
    CallBuffers cb;
    cb.open(device);
    const double* dx1 = cb.put(x1, 2 * (size_t)N);
    const double* dx2 = cb.put(x2, 2 * (size_t)N);
    double* dX = cb.get<double>(4 * (size_t)N);
    double* de = cb.get<double>(2 * (size_t)N);
    TriCams cams;
    std::memcpy(cams.P1, P1, sizeof(cams.P1)); std::memcpy(cams.P2, P2, sizeof(cams.P2));
    hipLaunchKernelGGL(k_triangulate, fit_blocks(N), dim3(256), 0, cb.st, cams, (long long)N, dx1, dx2, dX,
                       err1 ? de : (double*)nullptr, err2 ? de + N : (double*)nullptr);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(X, dX, sizeof(double) * 4 * N, hipMemcpyDeviceToHost, cb.st));
    if (err1) MVUS_HIP(hipMemcpyAsync(err1, de, sizeof(double) * N, hipMemcpyDeviceToHost, cb.st));
    if (err2) MVUS_HIP(hipMemcpyAsync(err2, de + N, sizeof(double) * N, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    return MVUS_OK;
  });
}

int mvus_triangulate_cov(int32_t device, int64_t N, const double* x1, const double* x2, const double* P1, const double* P2, double sigma1,
                         double sigma2, double* X, double* cov, double* err1, double* err2) {
  if (N < 0 || !P1 || !P2 || (N > 0 && (!x1 || !x2 || !X))) { g_create_error = "triangulate_cov: bad arguments"; return MVUS_E_INVALID; }
  if (!cov) { g_create_error = "triangulate_cov: cov is NULL (mvus_triangulate is the call without a covariance)"; return MVUS_E_INVALID; }
  if (!std::isfinite(sigma1) || !std::isfinite(sigma2) || !(sigma1 > 0.0) || !(sigma2 > 0.0)) {
    g_create_error = "triangulate_cov: sigma1 and sigma2 must be finite and > 0";
    return MVUS_E_INVALID;
  }
  if (N == 0) return MVUS_OK;
  return stateless([&] {
    CallBuffers cb;
    cb.open(device);
    const double* dx1 = cb.put(x1, 2 * (size_t)N);
    const double* dx2 = cb.put(x2, 2 * (size_t)N);
    double* dX = cb.get<double>(4 * (size_t)N);
    double* dC = cb.get<double>(6 * (size_t)N);
    double* de = cb.get<double>(2 * (size_t)N);
    TriCams cams;
    std::memcpy(cams.P1, P1, sizeof(cams.P1)); std::memcpy(cams.P2, P2, sizeof(cams.P2));
    hipLaunchKernelGGL(k_triangulate_cov, fit_blocks(N), dim3(256), 0, cb.st, cams, sigma1, sigma2, (long long)N, dx1, dx2, dX, dC,
                       err1 ? de : (double*)nullptr, err2 ? de + N : (double*)nullptr);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(X, dX, sizeof(double) * 4 * N, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(cov, dC, sizeof(double) * 6 * N, hipMemcpyDeviceToHost, cb.st));
    if (err1) MVUS_HIP(hipMemcpyAsync(err1, de, sizeof(double) * N, hipMemcpyDeviceToHost, cb.st));
    if (err2) MVUS_HIP(hipMemcpyAsync(err2, de + N, sizeof(double) * N, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    return MVUS_OK;
  });
}

/* cv2.solvePnPRansac(objectPoints, imagePoints, K, d, reprojectionError) as Scene.get_camera_pose calls it (pnp.hip.h) */
int mvus_pnp_ransac(int32_t device, int64_t N, const double* X, const double* uv, const double* K, const double* d, double reproj_error,
                    int32_t iterations, uint64_t seed, double* rvec, double* tvec, uint8_t* inliers, int64_t* n_inliers) {
  if (N < 6 || N > (1ll << 30) || !X || !uv || !K || !d || !rvec || !tvec || !(reproj_error > 0.0) || iterations < 1 || iterations > 65536) {
    g_create_error = "pnp_ransac: bad arguments (at least 6 points, reprojection error > 0, 1..65536 iterations)";
    return MVUS_E_INVALID;
  }
  for (int64_t i = 0; i < 3 * N; ++i) if (!std::isfinite(X[i])) { g_create_error = "pnp_ransac: non-finite object point"; return MVUS_E_INVALID; }
  for (int64_t i = 0; i < 2 * N; ++i) if (!std::isfinite(uv[i])) { g_create_error = "pnp_ransac: non-finite image point"; return MVUS_E_INVALID; }
  // the object points are centred and scaled (the direct linear transform is badly conditioned otherwise); a pose (R, t')
  // of the scaled points is the pose (R, sigma t' - R m) of the original ones
  return stateless([&] {
    double m[3] = {0.0, 0.0, 0.0}, sigma = 0.0;
    for (int a = 0; a < 3; ++a) { for (int64_t i = 0; i < N; ++i) m[a] += X[a * N + i]; m[a] /= (double)N; }
    for (int a = 0; a < 3; ++a) for (int64_t i = 0; i < N; ++i) sigma += (X[a * N + i] - m[a]) * (X[a * N + i] - m[a]);
    sigma = std::sqrt(sigma / (3.0 * (double)N));
    if (!(sigma > 0.0)) { g_create_error = "pnp_ransac: all object points coincide"; return MVUS_E_INVALID; }
    std::vector<double> Xc(3 * (size_t)N);
    for (int a = 0; a < 3; ++a) for (int64_t i = 0; i < N; ++i) Xc[a * N + i] = (X[a * N + i] - m[a]) / sigma;
    double Kd[9] = {K[0], K[1], K[2], K[3], d[0], d[1], d[2], d[3], d[4]};
    CallBuffers cb;
    cb.open(device);
    const double* dX = cb.put(Xc.data(), Xc.size());
    const double* duv = cb.put(uv, 2 * (size_t)N);
    const double* dK = cb.put(Kd, 9);
    double* xn = cb.get<double>(2 * (size_t)N);
    double* poses = cb.get<double>(13 * (size_t)iterations);
    int32_t* counts = cb.get<int32_t>((size_t)iterations);
    uint8_t* mask = cb.get<uint8_t>((size_t)N);
    double* pose_d = cb.get<double>(13);
    double* acc_d = cb.get<double>(29);
    const double thr2 = reproj_error * reproj_error;
    hipLaunchKernelGGL(k_pnp_normalise, fit_blocks(N), dim3(256), 0, cb.st, (long long)N, duv, dK, xn);
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3((iterations + 63) / 64), dim3(64), 0, cb.st, iterations, (unsigned long long)seed, (long long)N, dX, xn, poses);
    hipLaunchKernelGGL(k_pnp_score, dim3(iterations), dim3(256), 0, cb.st, (long long)N, dX, duv, dK, poses, thr2, counts);
    MVUS_HIP(hipGetLastError());
    std::vector<int32_t> cnt((size_t)iterations);
    MVUS_HIP(hipMemcpyAsync(cnt.data(), counts, sizeof(int32_t) * iterations, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    int best = 0;
    for (int h = 1; h < iterations; ++h) if (cnt[h] > cnt[best]) best = h;          // ties: the first hypothesis
    if (cnt[best] < 6) { g_create_error = "pnp_ransac: no hypothesis is supported by six points (reprojection error too small, or no consistent pose)"; return MVUS_E_NUMERIC; }
    double pose[13];
    MVUS_HIP(hipMemcpyAsync(pose, poses + 13ll * best, sizeof(double) * 13, hipMemcpyDeviceToHost, cb.st));
    hipLaunchKernelGGL(k_pnp_mask, fit_blocks(N), dim3(256), 0, cb.st, (long long)N, dX, duv, dK, poses + 13ll * best, thr2, mask);
    MVUS_HIP(hipStreamSynchronize(cb.st));
    // damped Gauss-Newton on the inliers; the normal equations come from the device, the 6x6 solve is done here
    double acc[29], cand[13], acc2[29];
    auto evaluate = [&](const double* ps, double* out) {
      MVUS_HIP(hipMemcpyAsync(pose_d, ps, sizeof(double) * 13, hipMemcpyHostToDevice, cb.st));
      hipLaunchKernelGGL(k_pnp_normal, dim3(1), dim3(256), 0, cb.st, (long long)N, dX, duv, dK, pose_d, mask, acc_d);
      MVUS_HIP(hipMemcpyAsync(out, acc_d, sizeof(double) * 29, hipMemcpyDeviceToHost, cb.st));
      MVUS_HIP(hipStreamSynchronize(cb.st));
    };
    evaluate(pose, acc);
    double lambda = 1e-3;
    for (int it = 0; it < 100; ++it) {
      double Hm[6][6], g[6], L[6][6], dlt[6];
      int e = 0;
      for (int a = 0; a < 6; ++a) for (int b = 0; b <= a; ++b) { Hm[a][b] = Hm[b][a] = acc[e++]; }
      for (int a = 0; a < 6; ++a) { g[a] = acc[21 + a]; Hm[a][a] += lambda * (Hm[a][a] > 0.0 ? Hm[a][a] : 1.0); }
      bool pd = true;
      for (int j = 0; j < 6 && pd; ++j) {
        double s = Hm[j][j];
        for (int k2 = 0; k2 < j; ++k2) s -= L[j][k2] * L[j][k2];
        if (!(s > 0.0)) { pd = false; break; }
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < 6; ++i) { double v = Hm[i][j]; for (int k2 = 0; k2 < j; ++k2) v -= L[i][k2] * L[j][k2]; L[i][j] = v / L[j][j]; }
      }
      if (!pd) { lambda *= 10.0; if (lambda > 1e10) break; continue; }
      for (int i = 0; i < 6; ++i) { double v = -g[i]; for (int k2 = 0; k2 < i; ++k2) v -= L[i][k2] * dlt[k2]; dlt[i] = v / L[i][i]; }
      for (int i = 5; i >= 0; --i) { double v = dlt[i]; for (int k2 = i + 1; k2 < 6; ++k2) v -= L[k2][i] * dlt[k2]; dlt[i] = v / L[i][i]; }
      double dR[9], W[9];
      rodrigues(dlt, dR, W);
      for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) cand[3 * a + b] = dR[3 * a] * pose[b] + dR[3 * a + 1] * pose[3 + b] + dR[3 * a + 2] * pose[6 + b];
      for (int a = 0; a < 3; ++a) cand[9 + a] = pose[9 + a] + dlt[3 + a];
      cand[12] = 1.0;
      evaluate(cand, acc2);
      double step = 0.0;
      for (int a = 0; a < 6; ++a) step = std::max(step, std::fabs(dlt[a]));
      if (acc2[28] == 0.0 && acc2[27] <= acc[27]) {
        const double gain = acc[27] - acc2[27];
        std::memcpy(pose, cand, sizeof(pose));
        std::memcpy(acc, acc2, sizeof(acc));
        lambda = std::max(lambda * 0.1, 1e-12);
        if (step < 1e-13 || gain <= 1e-15 * acc[27]) break;
      } else {
        lambda *= 10.0;
        if (lambda > 1e10 || step < 1e-14) break;
      }
    }
    // back to the scale of the original points
    for (int a = 0; a < 3; ++a) tvec[a] = sigma * pose[9 + a] - (pose[3 * a] * m[0] + pose[3 * a + 1] * m[1] + pose[3 * a + 2] * m[2]);
    rotation_to_rvec(pose, rvec);
    if (inliers) MVUS_HIP(hipMemcpyAsync(inliers, mask, (size_t)N, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    if (n_inliers) *n_inliers = cnt[best];
    return MVUS_OK;
  });
}

int mvus_fundamental_ransac(int32_t device, int32_t P, const int64_t* offsets, const double* x1, const double* x2, double thresh,
                            int32_t iterations, uint64_t seed, double* F_out, uint8_t* mask, int32_t* n_inliers) {
  if (P < 1 || !offsets || !x1 || !x2 || !F_out || !mask || !(thresh > 0.0) || !std::isfinite(thresh) || iterations < 1 || iterations > 65536)
    return epi_fail("fundamental_ransac: bad arguments (P >= 1, thresh > 0, 1..65536 iterations)", MVUS_E_INVALID);
  if (offsets[0] != 0) return epi_fail("fundamental_ransac: offsets[0] must be 0", MVUS_E_INVALID);
  for (int p = 0; p < P; ++p)
    if (offsets[p + 1] - offsets[p] < 8) return epi_fail("fundamental_ransac: every problem needs at least 8 pairs", MVUS_E_INVALID);
  const int64_t Ntot = offsets[P];
  if (Ntot > (1ll << 31)) return epi_fail("fundamental_ransac: more than 2^31 pairs", MVUS_E_INVALID);
  for (int64_t i = 0; i < 2 * Ntot; ++i)
    if (!std::isfinite(x1[i]) || !std::isfinite(x2[i])) return epi_fail("fundamental_ransac: non-finite point", MVUS_E_INVALID);
  const int H = iterations, M = kFmSlots * H, B = kFmRefitBlocks;
  const double thr2 = thresh * thresh;
  return stateless([&] {
    CallBuffers cb;
    cb.open(device);
    const long long* doffs = reinterpret_cast<const long long*>(cb.put(offsets, (size_t)P + 1));
    const double* dx1 = cb.put(x1, 2 * (size_t)Ntot);
    const double* dx2 = cb.put(x2, 2 * (size_t)Ntot);
    double* norm = cb.get<double>(6 * (size_t)P);
    double* models = cb.get<double>((size_t)P * M * kFmModel);
    int32_t* counts = cb.get<int32_t>((size_t)P * M);
    double* dF = cb.get<double>(9 * (size_t)P);
    uint8_t* mwin = cb.get<uint8_t>((size_t)Ntot);
    uint8_t* mref = cb.get<uint8_t>((size_t)Ntot);
    double* parts = cb.get<double>((size_t)P * B * 45);
    int32_t* rcnt = cb.get<int32_t>((size_t)P * B);
    hipLaunchKernelGGL(k_fm_normalise, dim3(P), dim3(256), 0, cb.st, doffs, (long long)Ntot, dx1, dx2, norm);
    hipLaunchKernelGGL(k_fm_hypotheses, dim3((H + 63) / 64, P), dim3(64), 0, cb.st, H, (unsigned long long)seed, doffs, (long long)Ntot, dx1, dx2, norm, models);
    hipLaunchKernelGGL(k_fm_score, dim3((M + 255) / 256, P), dim3(256), 0, cb.st, H, doffs, (long long)Ntot, dx1, dx2, models, thr2, counts);
    MVUS_HIP(hipGetLastError());
    std::vector<int32_t> cnt((size_t)P * M);
    std::vector<double> nrm(6 * (size_t)P);
    MVUS_HIP(hipMemcpyAsync(cnt.data(), counts, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(nrm.data(), norm, sizeof(double) * nrm.size(), hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    // the winner of every problem: highest count, lowest model index on ties
    std::vector<double> Fw(9 * (size_t)P), Fr(9 * (size_t)P);
    std::vector<int32_t> best_cnt(P);
    for (int p = 0; p < P; ++p) {
      const int32_t* c = cnt.data() + (size_t)p * M;
      int best = 0;
      for (int m = 1; m < M; ++m) if (c[m] > c[best]) best = m;
      if (c[best] < 0) return epi_fail("fundamental_ransac: no valid 7-point model (degenerate configuration)", MVUS_E_NUMERIC);
      best_cnt[p] = c[best];
      MVUS_HIP(hipMemcpyAsync(Fw.data() + 9 * (size_t)p, models + ((size_t)p * M + best) * kFmModel, sizeof(double) * 9, hipMemcpyDeviceToHost, cb.st));
    }
    MVUS_HIP(hipStreamSynchronize(cb.st));
    MVUS_HIP(hipMemcpyAsync(dF, Fw.data(), sizeof(double) * 9 * P, hipMemcpyHostToDevice, cb.st));
    hipLaunchKernelGGL(k_fm_refit, dim3(B, P), dim3(256), 0, cb.st, doffs, (long long)Ntot, dx1, dx2, norm, dF, thr2, mwin, parts);
    MVUS_HIP(hipGetLastError());
    std::vector<double> hp((size_t)P * B * 45);
    MVUS_HIP(hipMemcpyAsync(hp.data(), parts, sizeof(double) * hp.size(), hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    // normalised 8-point refit on the winner's inliers: smallest eigenvector of the normal matrix, rank 2, denormalised
    std::vector<char> have_refit(P, 0);
    for (int p = 0; p < P; ++p) {
      double Mx[81], w[9], V[81], Fn[9];
      double up[45];
      for (int e = 0; e < 45; ++e) { double s = 0.0; for (int b = 0; b < B; ++b) s += hp[((size_t)p * B + b) * 45 + e]; up[e] = s; }
      int e = 0;
      for (int a = 0; a < 9; ++a) for (int b = a; b < 9; ++b) { Mx[9 * a + b] = Mx[9 * b + a] = up[e++]; }
      if (best_cnt[p] < 8) { std::memcpy(Fr.data() + 9 * (size_t)p, Fw.data() + 9 * (size_t)p, sizeof(double) * 9); continue; }
      sym_eig_jacobi(9, Mx, w, V);
      for (int a = 0; a < 9; ++a) Fn[a] = V[9 * a];
      rank2(Fn);
      double Fd[9];
      fm_denormalise(Fn, nrm.data() + 6 * (size_t)p, Fd);
      bool ok = true;
      for (int a = 0; a < 9; ++a) ok = ok && std::isfinite(Fd[a]);
      std::memcpy(Fr.data() + 9 * (size_t)p, ok ? Fd : Fw.data() + 9 * (size_t)p, sizeof(double) * 9);
      have_refit[p] = ok ? 1 : 0;
    }
    MVUS_HIP(hipMemcpyAsync(dF, Fr.data(), sizeof(double) * 9 * P, hipMemcpyHostToDevice, cb.st));
    hipLaunchKernelGGL(k_fm_mask, dim3(B, P), dim3(256), 0, cb.st, doffs, (long long)Ntot, dx1, dx2, dF, thr2, mref, rcnt);
    MVUS_HIP(hipGetLastError());
    std::vector<int32_t> rc((size_t)P * B);
    std::vector<uint8_t> hw((size_t)Ntot);
    MVUS_HIP(hipMemcpyAsync(rc.data(), rcnt, sizeof(int32_t) * rc.size(), hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(hw.data(), mwin, (size_t)Ntot, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(mask, mref, (size_t)Ntot, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    for (int p = 0; p < P; ++p) {
      int32_t c = 0;
      for (int b = 0; b < B; ++b) c += rc[(size_t)p * B + b];
      const bool refit = have_refit[p] && c >= best_cnt[p];
      std::memcpy(F_out + 9 * (size_t)p, (refit ? Fr : Fw).data() + 9 * (size_t)p, sizeof(double) * 9);
      if (!refit) std::memcpy(mask + offsets[p], hw.data() + offsets[p], (size_t)(offsets[p + 1] - offsets[p]));
      if (n_inliers) n_inliers[p] = refit ? c : best_cnt[p];
    }
    return MVUS_OK;
  });
}

int mvus_correct_matches(int32_t device, int64_t N, const double* F, const double* x1, const double* x2, double* x1c, double* x2c) {
  if (N < 0 || !F || (N > 0 && (!x1 || !x2 || !x1c || !x2c))) return epi_fail("correct_matches: bad arguments", MVUS_E_INVALID);
  double nn = 0.0;
  for (int a = 0; a < 9; ++a) { if (!std::isfinite(F[a])) return epi_fail("correct_matches: F is not finite", MVUS_E_INVALID); nn += F[a] * F[a]; }
  if (!(nn > 0.0)) return epi_fail("correct_matches: F is zero", MVUS_E_INVALID);
  if (N == 0) return MVUS_OK;
  return stateless([&] {
    EpiF f;
    for (int a = 0; a < 9; ++a) f.F[a] = F[a] / std::sqrt(nn);
    null3_cross(f.F, false, f.e1);
    null3_cross(f.F, true, f.e2);
    CallBuffers cb;
    cb.open(device);
    const double* dx1 = cb.put(x1, 2 * (size_t)N);
    const double* dx2 = cb.put(x2, 2 * (size_t)N);
    double* o1 = cb.get<double>(2 * (size_t)N);
    double* o2 = cb.get<double>(2 * (size_t)N);
    hipLaunchKernelGGL(k_correct_matches, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, cb.st, f, (long long)N, dx1, dx2, o1, o2);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(x1c, o1, sizeof(double) * 2 * N, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(x2c, o2, sizeof(double) * 2 * N, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    return MVUS_OK;
  });
}

int mvus_pose_from_essential(int32_t device, int64_t N, const double* E, const double* x1n, const double* x2n, double* P2_out, double* X_out) {
  if (N < 1 || N > (1ll << 31) || !E || !x1n || !x2n || !P2_out || !X_out) return epi_fail("pose_from_essential: bad arguments (N >= 1)", MVUS_E_INVALID);
  for (int a = 0; a < 9; ++a) if (!std::isfinite(E[a])) return epi_fail("pose_from_essential: E is not finite", MVUS_E_INVALID);
  for (int64_t i = 0; i < 2 * N; ++i)
    if (!std::isfinite(x1n[i]) || !std::isfinite(x2n[i])) return epi_fail("pose_from_essential: non-finite point", MVUS_E_INVALID);
  return stateless([&] {
    EpiCand cand;
    essential_candidates(E, cand.P2);
    for (int c = 0; c < 4; ++c) for (int a = 0; a < 12; ++a)
      if (!std::isfinite(cand.P2[c][a])) return epi_fail("pose_from_essential: E has no valid decomposition", MVUS_E_NUMERIC);
    const int B = (int)std::min<long long>(64, (N + 255) / 256);
    CallBuffers cb;
    cb.open(device);
    const double* dx1 = cb.put(x1n, 2 * (size_t)N);
    const double* dx2 = cb.put(x2n, 2 * (size_t)N);
    int32_t* dcnt = cb.get<int32_t>(4 * (size_t)B);
    double* dX = cb.get<double>(4 * (size_t)N);
    hipLaunchKernelGGL(k_cheirality4, dim3(B, 4), dim3(256), 0, cb.st, cand, (long long)N, dx1, dx2, dcnt);
    MVUS_HIP(hipGetLastError());
    std::vector<int32_t> hc(4 * (size_t)B);
    MVUS_HIP(hipMemcpyAsync(hc.data(), dcnt, sizeof(int32_t) * hc.size(), hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    long long infront_max = 0;
    int chosen = -1;
    for (int c = 0; c < 4; ++c) {
      long long s = 0;
      for (int b = 0; b < B; ++b) s += hc[(size_t)c * B + b];
      if (s > infront_max) { infront_max = s; chosen = c; }          // strict: the first candidate to exceed the running maximum
    }
    if (chosen < 0) return epi_fail("pose_from_essential: no candidate puts a point in front of a camera", MVUS_E_NUMERIC);
    TriCams cams;
    const double I34[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    std::memcpy(cams.P1, I34, sizeof(I34));
    std::memcpy(cams.P2, cand.P2[chosen], sizeof(cams.P2));
    hipLaunchKernelGGL(k_triangulate, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, cb.st, cams, (long long)N, dx1, dx2, dX,
                       (double*)nullptr, (double*)nullptr);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(X_out, dX, sizeof(double) * 4 * N, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    std::memcpy(P2_out, cand.P2[chosen], sizeof(double) * 12);
    return MVUS_OK;
  });
}

// ---- iterative time-shift search (sync_iter.hip.h) ---------------------------------------------------------------------------
namespace {
bool si_all_finite(const double* x, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false; return true; }
bool si_knots_ok(int n, const double* t) {
  if (n < 4 || !si_all_finite(t, (size_t)n + 4)) return false;
  for (int i = 0; i + 1 < n + 4; ++i) if (t[i] > t[i + 1]) return false;
  return t[3] < t[n];
}
// the score of the session's first `count` models: counts zeroed, one workgroup per (model, tile)
void si_launch_score(mvus_sync_iter* S, double shift, long long count, double threshold) {
  MVUS_HIP(hipMemsetAsync(S->counts, 0, sizeof(int32_t) * 2 * count, S->st));
  const unsigned tiles = (unsigned)((S->v.N1 + kSiScoreTile - 1) / kSiScoreTile);
  hipLaunchKernelGGL(k_si_score, dim3((unsigned)count, tiles), dim3(256), 0, S->st, S->v, shift, S->models, threshold, S->counts);
}
constexpr int kSiMaxHyp = 1 << 20;
}  // namespace

int mvus_sync_iter_open(int32_t device, int32_t n1, const double* knots1, const double* coef1, int32_t n2, const double* knots2, const double* coef2,
                        int32_t K, const double* intervals2, int64_t N1, const double* detect1, int64_t N2, const double* t2, mvus_sync_iter** out) {
  if (!out) return epi_fail("sync_iter_open: bad arguments", MVUS_E_INVALID);
  *out = nullptr;
  if (!knots1 || !coef1 || !knots2 || !coef2 || K < 0 || (K > 0 && !intervals2) || N1 < 1 || N2 < 1 || N1 > (1ll << 30) || N2 > (1ll << 30) || !detect1 || !t2)
    return epi_fail("sync_iter_open: bad arguments (two splines, K >= 0 intervals, at least one sample per camera)", MVUS_E_INVALID);
  if (!si_knots_ok(n1, knots1) || !si_knots_ok(n2, knots2))
    return epi_fail("sync_iter_open: a spline needs at least 4 coefficients and finite ascending knots", MVUS_E_INVALID);
  if (!si_all_finite(coef1, 2 * (size_t)n1) || !si_all_finite(coef2, 2 * (size_t)n2)) return epi_fail("sync_iter_open: non-finite spline coefficient", MVUS_E_INVALID);
  mvus_sync_iter* S = nullptr;
  try { S = new mvus_sync_iter(); } catch (const std::exception& e) { g_create_error = e.what(); return MVUS_E_INVALID; }
  const int rc = stateless([&] {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) throw HipError{"no usable HIP device (libmvusba has no CPU fallback)"};
    S->device = device;
    MVUS_HIP(hipSetDevice(device));
    MVUS_HIP(hipStreamCreateWithFlags(&S->st, hipStreamNonBlocking));
    SiView& v = S->v;
    v.n1 = n1; v.n2 = n2; v.K = K; v.N1 = N1; v.N2 = N2;
    v.t1k = S->put(knots1, (size_t)n1 + 4); v.c1 = S->put(coef1, 2 * (size_t)n1);
    v.t2k = S->put(knots2, (size_t)n2 + 4); v.c2 = S->put(coef2, 2 * (size_t)n2);
    v.iv = S->put(intervals2, 2 * (size_t)K);
    v.d1 = S->put(detect1, 3 * (size_t)N1);
    v.t2 = S->put(t2, (size_t)N2);
    MVUS_HIP(hipStreamSynchronize(S->st));
    return MVUS_OK;
  });
  if (rc != MVUS_OK) { delete S; return rc; }
  *out = S;
  return MVUS_OK;
}

void mvus_sync_iter_close(mvus_sync_iter* S) { delete S; }

int mvus_sync_iter_round(mvus_sync_iter* S, double shift, int32_t d, int32_t H, double threshold, uint64_t seed, int32_t round, double* out) {
  if (!S || !out || H < 1 || H > kSiMaxHyp || d == 0 || d == INT32_MIN || !std::isfinite(shift) || !(threshold > 0.0) || round < 0)
    return epi_fail("sync_iter_round: bad arguments (a session, H >= 1, d != 0, finite shift, threshold > 0)", MVUS_E_INVALID);
  const long long n = std::min(S->v.N1, S->v.N2) - 2ll * std::llabs((long long)d);
  if (n < kSiSample) return epi_fail("sync_iter_round: fewer than nine samples to draw from (min(N1, N2) - 2 |d| < 9)", MVUS_E_INVALID);
  return stateless([&] {
    MVUS_HIP(hipSetDevice(S->device));
    const long long Mper = (long long)H * kSiSlots;
    S->reserve(2ll * H, 2 * Mper);
    hipLaunchKernelGGL(k_si_hypotheses, dim3((H + 63) / 64, 2), dim3(64), 0, S->st, S->v, shift, (int)d, (int)H, (unsigned long long)seed, (int)round, n,
                       (const long long*)nullptr, S->samp, S->betas, S->valid);
    hipLaunchKernelGGL(k_si_models, dim3((unsigned)((2 * Mper + 63) / 64)), dim3(64), 0, S->st, (int)d, (int)H, 2, S->samp, S->betas, S->valid, S->models);
    si_launch_score(S, shift, 2 * Mper, threshold);
    hipLaunchKernelGGL(k_si_select, dim3(2), dim3(256), 0, S->st, Mper, S->models, S->counts, S->out);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(out, S->out, sizeof(double) * 8, hipMemcpyDeviceToHost, S->st));
    MVUS_HIP(hipStreamSynchronize(S->st));
    return MVUS_OK;
  });
}

int mvus_sync_iter_models(mvus_sync_iter* S, double shift, int32_t d, int32_t H, const int64_t* idx, double threshold, double* betas, uint8_t* valid,
                          double* F, int32_t* counts) {
  if (!S || !idx || !betas || !valid || !F || !counts || H < 1 || H > kSiMaxHyp || d == 0 || d == INT32_MIN || !std::isfinite(shift) || !(threshold > 0.0))
    return epi_fail("sync_iter_models: bad arguments (a session, H >= 1, d != 0, finite shift, threshold > 0)", MVUS_E_INVALID);
  for (int64_t i = 0; i < (int64_t)H * kSiSample; ++i)
    if (idx[i] < 0 || idx[i] >= S->v.N2) return epi_fail("sync_iter_models: sample index outside camera 2's detections", MVUS_E_INVALID);
  return stateless([&] {
    MVUS_HIP(hipSetDevice(S->device));
    const long long Mper = (long long)H * kSiSlots;
    S->reserve(H, Mper);
    static_assert(sizeof(long long) == sizeof(int64_t), "index width");
    MVUS_HIP(hipMemcpyAsync(S->idx, idx, sizeof(int64_t) * H * kSiSample, hipMemcpyHostToDevice, S->st));
    // (d carries its own sign here: one sign, the hypotheses of blockIdx.y = 0)
    hipLaunchKernelGGL(k_si_hypotheses, dim3((H + 63) / 64, 1), dim3(64), 0, S->st, S->v, shift, (int)d, (int)H, 0ull, 0, (long long)S->v.N2,
                       (const long long*)S->idx, S->samp, S->betas, S->valid);
    hipLaunchKernelGGL(k_si_models, dim3((unsigned)((Mper + 63) / 64)), dim3(64), 0, S->st, (int)d, (int)H, 1, S->samp, S->betas, S->valid, S->models);
    si_launch_score(S, shift, Mper, threshold);
    MVUS_HIP(hipGetLastError());
    std::vector<double> hm((size_t)Mper * kSiModel);
    MVUS_HIP(hipMemcpyAsync(hm.data(), S->models, sizeof(double) * hm.size(), hipMemcpyDeviceToHost, S->st));
    MVUS_HIP(hipMemcpyAsync(betas, S->betas, sizeof(double) * Mper, hipMemcpyDeviceToHost, S->st));
    MVUS_HIP(hipMemcpyAsync(valid, S->valid, (size_t)Mper, hipMemcpyDeviceToHost, S->st));
    MVUS_HIP(hipMemcpyAsync(counts, S->counts, sizeof(int32_t) * 2 * Mper, hipMemcpyDeviceToHost, S->st));
    MVUS_HIP(hipStreamSynchronize(S->st));
    for (long long m = 0; m < Mper; ++m) std::memcpy(F + 9 * m, hm.data() + kSiModel * m, sizeof(double) * 9);
    return MVUS_OK;
  });
}

int mvus_sync_iter_score(mvus_sync_iter* S, double shift, int64_t M, const double* models, double threshold, int32_t* counts) {
  if (!S || M < 0 || M > (1ll << 24) || (M > 0 && (!models || !counts)) || !std::isfinite(shift) || !(threshold > 0.0))
    return epi_fail("sync_iter_score: bad arguments (a session, 0 <= M <= 2^24 models, finite shift, threshold > 0)", MVUS_E_INVALID);
  if (M == 0) return MVUS_OK;
  return stateless([&] {
    MVUS_HIP(hipSetDevice(S->device));
    S->reserve(0, M);
    // a model handed in is scored when its flag is set and its eleven numbers are finite
    std::vector<double> hm(models, models + (size_t)M * kSiModel);
    for (int64_t m = 0; m < M; ++m) {
      bool ok = hm[kSiModel * m + 10] != 0.0;
      for (int a = 0; a < kSiModel; ++a) ok = ok && std::isfinite(hm[kSiModel * m + a]);
      hm[kSiModel * m + 10] = ok ? 1.0 : 0.0;
    }
    MVUS_HIP(hipMemcpyAsync(S->models, hm.data(), sizeof(double) * hm.size(), hipMemcpyHostToDevice, S->st));
    si_launch_score(S, shift, M, threshold);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(counts, S->counts, sizeof(int32_t) * 2 * M, hipMemcpyDeviceToHost, S->st));
    MVUS_HIP(hipStreamSynchronize(S->st));
    return MVUS_OK;
  });
}

}  // extern "C"
