// libmvusba.so, spline stage: evaluation, least-squares fit and the FITPACK smoothing fit (mvus_spline_* of include/mvus_ba.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "api_common.h"
#include "spline_ops.hip.h"
#include "spline_fit.hip.h"

using namespace mvus;

// device work arrays of the smoothing fit in one precision (double, or double-double for ill-conditioned knot sets)
template <class T>
struct FitWork {
  T *SB = nullptr, *G5 = nullptr, *BtB = nullptr, *Mx = nullptr, *Lf = nullptr, *rhs = nullptr, *yw = nullptr, *YL = nullptr, *parts = nullptr;
  bool ready = false, penalty = false;
  void alloc(CallBuffers& cb, size_t nest) {
    if (ready) return;
    SB = cb.get<T>((size_t)kFitBlk * (nest + kFitSliceBlocks)); G5 = cb.get<T>(5 * nest); BtB = cb.get<T>(5 * nest); Mx = cb.get<T>(5 * nest);
    const size_t rows = nest + kBandPartsMax;            // the transposed copies hold length(0) rows for EVERY interior
    Lf = cb.get<T>(5 * rows); rhs = cb.get<T>(3 * nest); yw = cb.get<T>(3 * rows);
    YL = cb.get<T>(4 * rows); parts = cb.get<T>((size_t)kBandPartsWork);
    ready = true;
  }
};
// systems of at least this many rows go to k_band_solve_parts (MVUS_BAND_PARTS_MIN: the tests push the small fixtures through it too)
static int band_parts_min() {
  static const int v = [] { const char* e = std::getenv("MVUS_BAND_PARTS_MIN"); return e ? std::max(16, std::atoi(e)) : 192; }();
  return v;
}
// banded solve of the pass; returns true when the factor's diagonal in out[0] is FITPACK's (one chain in the natural order)
template <int HB, class T>
static bool fit_band_solve(hipStream_t st, FitWork<T>& w, int ncoef, const BandParts& bp, const T* Mband, double* cd, double* out, int* fail) {
  if (bp.P < 2) {
    hipLaunchKernelGGL((k_band_solve<HB, T>), dim3(1), dim3(64), 0, st, ncoef, Mband, w.rhs, w.Lf, w.yw, cd, out, fail);
    return true;
  }
  hipLaunchKernelGGL((k_band_solve_parts<HB, T>), dim3(1), dim3(64 * ((bp.P + 63) / 64)), 0, st, ncoef, bp, Mband, w.rhs, w.Lf, w.yw, w.YL, w.parts, cd, out, fail);
  return false;
}
template <int HB, class T>
static bool fit_band_solve(hipStream_t st, FitWork<T>& w, int ncoef, const T* Mband, double* cd, double* out, int* fail) {
  return fit_band_solve<HB, T>(st, w, ncoef, band_parts(ncoef, HB, band_parts_min()), Mband, cd, out, fail);
}
// least-squares spline on the current knots: normal equations from the span blocks, banded Cholesky, coefficients -> cd
// (nslice slices per span -- the fit passes fit_slices(nrint) -- and the partition bp of the solve: band_parts(ncoef, 3, band_parts_min());
// wt: the weights of a weighted fit on the device, or NULL -- then the kernel that reads none)
template <class T>
static bool fit_lsq_pass(hipStream_t st, FitWork<T>& w, long long m, const long long* first, const double* q, const double* dX, const double* wt, int ncoef,
                         int nrint, int nslice, const BandParts& bp, double* cd, double* out, int* fail) {
  constexpr int NT = sizeof(T) == sizeof(double) ? 256 : 64;
  if (wt) hipLaunchKernelGGL((k_fit_blocks_w<T, NT>), dim3(nrint, nslice), dim3(NT), 0, st, m, first, q, dX, wt, w.SB);
  else hipLaunchKernelGGL((k_fit_blocks<T, NT>), dim3(nrint, nslice), dim3(NT), 0, st, m, first, q, dX, w.SB);
  if (nslice > 1) hipLaunchKernelGGL(k_fit_slice_sum<T>, fit_blocks((long long)nrint * kFitBlk), dim3(256), 0, st, (long long)nrint * kFitBlk, nslice, w.SB);
  hipLaunchKernelGGL(k_fit_band<T>, fit_blocks(ncoef), dim3(256), 0, st, ncoef, nrint, w.SB, w.G5, w.rhs, bp, w.Lf, w.yw);
  w.penalty = false;
  return fit_band_solve<3, T>(st, w, ncoef, bp, w.G5, cd, out, fail);
}
// c -> the squared residual of every sample (term), their total f_p (out[1]) and, with `spans`, the per-span sums (out[4 + sp]) in
// nslice slices per span (the fit passes fit_slices(nspan)); wt as in fit_lsq_pass: the residuals are then the weighted ones
static void fit_residual_pass(hipStream_t st, long long m, int ncoef, const int32_t* span, const double* q, const double* dX, const double* wt, const double* cd,
                              double* term, double* tot_part, double* out, bool spans, int nspan, int nslice, const long long* first, double* fp_part) {
  if (wt) hipLaunchKernelGGL(k_fit_residual_w, fit_blocks(m), dim3(256), 0, st, m, ncoef, span, q, dX, wt, cd, term);
  else hipLaunchKernelGGL(k_fit_residual, fit_blocks(m), dim3(256), 0, st, m, ncoef, span, q, dX, cd, term);
  if (m > kFitTotalOneStage) {                                    // two stages (still one fixed order)
    const int nbt = fit_total_parts(m);
    hipLaunchKernelGGL(k_fit_total_partial, dim3(nbt), dim3(256), 0, st, m, term, tot_part);
    hipLaunchKernelGGL(k_fit_total, dim3(1), dim3(256), 0, st, (long long)nbt, tot_part, out + 1);
  } else {
    hipLaunchKernelGGL(k_fit_total, dim3(1), dim3(256), 0, st, m, term, out + 1);
  }
  if (spans) {
    hipLaunchKernelGGL(k_fit_fpint, dim3(nspan, nslice), dim3(256), 0, st, nspan, first, term, out + 4, fp_part);
    if (nslice > 1) hipLaunchKernelGGL(k_fit_fpint_final, fit_blocks(nspan), dim3(256), 0, st, nspan, nslice, first, term, fp_part, out + 4);
  }
}
// the sum of the factor's diagonal in the natural elimination order (fppara's initial p) when the last pass was partitioned
template <class T>
static void fit_lsq_diag(hipStream_t st, FitWork<T>& w, int ncoef, double* out) {
  hipLaunchKernelGGL((k_band_diag_sum<3, T>), dim3(1), dim3(64), 0, st, ncoef, w.G5, out);
}
// smoothing spline for one value of p on the same knots (fit_lsq_pass has run in this precision)
template <class T>
static void fit_smooth_pass(hipStream_t st, FitWork<T>& w, int ncoef, int n8, const double* bd, double pinv, double* cd, double* out, int* fail) {
  if (!w.penalty) { hipLaunchKernelGGL(k_fit_penalty<T>, fit_blocks(ncoef), dim3(256), 0, st, ncoef, n8, bd, w.BtB); w.penalty = true; }
  hipLaunchKernelGGL(k_fit_combine<T>, fit_blocks(5ll * ncoef), dim3(256), 0, st, 5ll * ncoef, w.G5, w.BtB, pinv, w.Mx, ncoef, w.rhs,
                     band_parts(ncoef, 4, band_parts_min()), w.Lf, w.yw);
  fit_band_solve<4, T>(st, w, ncoef, w.Mx, cd, out, fail);
}

// ---- inspection: the band solvers on a system handed in (mvus_spline_band_solve, mvus_spline_band_diag_sum) ----------------------------
// `count` operands on the device as T: the high words alone in fp64, dd(hi, lo) in double-double (lo NULL: 0).  `stage` outlives the copy.
static void band_fill(CallBuffers& cb, double* dst, const double* hi, const double*, size_t count, std::vector<dd>&) {
  MVUS_HIP(hipMemcpyAsync(dst, hi, sizeof(double) * count, hipMemcpyHostToDevice, cb.st));
}
static void band_fill(CallBuffers& cb, dd* dst, const double* hi, const double* lo, size_t count, std::vector<dd>& stage) {
  stage.resize(count);
  for (size_t i = 0; i < count; ++i) stage[i] = dd(hi[i], lo ? lo[i] : 0.0);
  MVUS_HIP(hipMemcpyAsync(dst, stage.data(), sizeof(dd) * count, hipMemcpyHostToDevice, cb.st));
}
// the work arrays of a fit with nest = n (FitWork::alloc: the allocation rule is what the kernels index into), the system copied in, then
// what fit_lsq_pass (hb = 3) / fit_smooth_pass (hb = 4) launch after their assembly
template <class T>
static int band_solve_run(int32_t device, int n, int hb, const BandParts& bp, const double* G5, const double* G5_lo, const double* BtB, const double* BtB_lo,
                          double pinv, const double* rhs, const double* rhs_lo, double* c_out, double* stats_out, int32_t* fail_out) {
  CallBuffers cb;
  cb.open(device);
  FitWork<T> w;
  w.alloc(cb, (size_t)n);
  std::vector<dd> s_g, s_b, s_r;
  band_fill(cb, w.G5, G5, G5_lo, 5 * (size_t)n, s_g);
  band_fill(cb, w.rhs, rhs, rhs_lo, 3 * (size_t)n, s_r);
  if (hb == 4) band_fill(cb, w.BtB, BtB, BtB_lo, 5 * (size_t)n, s_b);
  double* cd = cb.get<double>(3 * (size_t)n);
  double* out = cb.get<double>(4);
  int* fail = cb.get<int>(1);
  const double unset = std::nan("");
  const double out0[4] = {unset, unset, unset, unset};       // out[0] stays NaN where the partitioned kernel does not write it
  MVUS_HIP(hipMemcpyAsync(out, out0, sizeof(out0), hipMemcpyHostToDevice, cb.st));
  MVUS_HIP(hipMemsetAsync(fail, 0, sizeof(int), cb.st));
  if (hb == 3) {
    if (bp.P > 1) hipLaunchKernelGGL(k_band_scatter<T>, fit_blocks(n), dim3(256), 0, cb.st, n, w.G5, w.rhs, bp, w.Lf, w.yw);
    fit_band_solve<3, T>(cb.st, w, n, bp, w.G5, cd, out, fail);
  } else {
    hipLaunchKernelGGL(k_fit_combine<T>, fit_blocks(5ll * n), dim3(256), 0, cb.st, 5ll * n, w.G5, w.BtB, pinv, w.Mx, n, w.rhs, bp, w.Lf, w.yw);
    fit_band_solve<4, T>(cb.st, w, n, bp, w.Mx, cd, out, fail);
  }
  MVUS_HIP(hipGetLastError());
  int fh = 0;
  MVUS_HIP(hipMemcpyAsync(c_out, cd, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipMemcpyAsync(stats_out, out, sizeof(double) * 4, hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipMemcpyAsync(&fh, fail, sizeof(int), hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipStreamSynchronize(cb.st));
  *fail_out = fh;
  return MVUS_OK;
}
template <class T>
static int band_diag_sum_run(int32_t device, int n, const double* G5, const double* G5_lo, double* out_host) {
  CallBuffers cb;
  cb.open(device);
  T* M = cb.get<T>(5 * (size_t)n);
  std::vector<dd> s_g;
  band_fill(cb, M, G5, G5_lo, 5 * (size_t)n, s_g);
  double* out = cb.get<double>(1);
  hipLaunchKernelGGL((k_band_diag_sum<3, T>), dim3(1), dim3(64), 0, cb.st, n, M, out);
  MVUS_HIP(hipGetLastError());
  MVUS_HIP(hipMemcpyAsync(out_host, out, sizeof(double), hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipStreamSynchronize(cb.st));
  return MVUS_OK;
}

// ---- inspection: the passes of the fit around those solvers (mvus_spline_fit_normal, _penalty, _residual) ----------------------------------
// `count` values of a work array back on the host as high and low words (lo may be NULL; 0 in fp64)
static void band_read(CallBuffers& cb, const double* src, double* hi, double* lo, size_t count) {
  MVUS_HIP(hipMemcpyAsync(hi, src, sizeof(double) * count, hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipStreamSynchronize(cb.st));
  if (lo) std::fill(lo, lo + count, 0.0);
}
static void band_read(CallBuffers& cb, const dd* src, double* hi, double* lo, size_t count) {
  std::vector<dd> stage(count);
  MVUS_HIP(hipMemcpyAsync(stage.data(), src, sizeof(dd) * count, hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipStreamSynchronize(cb.st));
  for (size_t i = 0; i < count; ++i) { hi[i] = stage[i].hi; if (lo) lo[i] = stage[i].lo; }
}
// what a weight vector must be (scipy's own condition on splprep's w); NULL: the unweighted fit
static const char* const kFitWeightsWrong = "the weights must be finite and strictly positive";
static bool fit_weights_ok(int64_t m, const double* w) {
  if (w) for (int64_t i = 0; i < m; ++i) if (!std::isfinite(w[i]) || !(w[i] > 0.0)) return false;
  return true;
}
// the checks the three share; slices: 0 the production rule, else exactly that many
static bool fit_inspect_args_ok(const char* name, int64_t m, const double* u, const double* X, const double* w, int32_t n, const double* t, int32_t slices) {
  if (const char* wrong = fit_samples_knots_wrong(m, u, n, t)) { g_create_error = std::string(name) + ": " + wrong; return false; }
  for (int64_t i = 0; i < 3 * m; ++i) if (!std::isfinite(X[i])) { g_create_error = std::string(name) + ": non-finite sample"; return false; }
  if (!fit_weights_ok(m, w)) { g_create_error = std::string(name) + ": " + kFitWeightsWrong; return false; }
  if (slices != 0 && !fit_slices_legal(n - 7, slices)) {
    g_create_error = std::string(name) + ": slices must be 0 (the production rule) or 1..256 with spans x (slices - 1) <= 1536 and spans x slices <= 2048";
    return false;
  }
  return true;
}
// samples and knots on the device, then what every pass of the fit starts with: k_fit_basis and k_fit_first
struct FitInputs {
  const double *du = nullptr, *dX = nullptr, *dw = nullptr, *td = nullptr;
  int32_t* span = nullptr;
  double* q = nullptr;
  long long* first = nullptr;
  void upload(CallBuffers& cb, int64_t m, const double* u, const double* X, const double* w, int n, const double* t) {
    const int ncoef = n - 4, nspan = n - 7;
    du = cb.put(u, (size_t)m); dX = cb.put(X, 3 * (size_t)m); td = cb.put(t, (size_t)n);
    if (w) dw = cb.put(w, (size_t)m);
    span = cb.get<int32_t>((size_t)m); q = cb.get<double>(4 * (size_t)m); first = cb.get<long long>((size_t)nspan + 1);
    hipLaunchKernelGGL(k_fit_basis, fit_blocks(m), dim3(256), 0, cb.st, (long long)m, du, td, ncoef, span, q);
    hipLaunchKernelGGL(k_fit_first, fit_blocks(nspan + 1), dim3(256), 0, cb.st, (long long)m, du, td, nspan, first);
  }
};
template <class T>
static int fit_normal_run(int32_t device, int64_t m, const double* u, const double* X, const double* wt, int n, const double* t, int slices, const BandParts& bp, int32_t* span_out,
                          double* q_out, int64_t* first_out, double* G5_out, double* G5_lo_out, double* rhs_out, double* rhs_lo_out, double* c_out,
                          double* stats_out, int32_t* fail_out) {
  const int ncoef = n - 4, nspan = n - 7;
  CallBuffers cb;
  cb.open(device);
  FitInputs in;
  in.upload(cb, m, u, X, wt, n, t);
  FitWork<T> w;
  w.alloc(cb, (size_t)n);
  double* cd = cb.get<double>(3 * (size_t)ncoef);
  double* out = cb.get<double>(4);
  int* fail = cb.get<int>(1);
  const double unset = std::nan("");
  const double out0[4] = {unset, unset, unset, unset};
  MVUS_HIP(hipMemcpyAsync(out, out0, sizeof(out0), hipMemcpyHostToDevice, cb.st));
  MVUS_HIP(hipMemsetAsync(fail, 0, sizeof(int), cb.st));
  fit_lsq_pass<T>(cb.st, w, (long long)m, in.first, in.q, in.dX, in.dw, ncoef, nspan, slices ? slices : fit_slices(nspan), bp, cd, out, fail);
  MVUS_HIP(hipGetLastError());
  int fh = 0;
  std::vector<long long> fh_first((size_t)nspan + 1);
  MVUS_HIP(hipMemcpyAsync(span_out, in.span, sizeof(int32_t) * m, hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipMemcpyAsync(q_out, in.q, sizeof(double) * 4 * m, hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipMemcpyAsync(fh_first.data(), in.first, sizeof(long long) * (nspan + 1), hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipMemcpyAsync(c_out, cd, sizeof(double) * 3 * ncoef, hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipMemcpyAsync(stats_out, out, sizeof(double) * 4, hipMemcpyDeviceToHost, cb.st));
  MVUS_HIP(hipMemcpyAsync(&fh, fail, sizeof(int), hipMemcpyDeviceToHost, cb.st));
  band_read(cb, w.G5, G5_out, G5_lo_out, 5 * (size_t)ncoef);
  band_read(cb, w.rhs, rhs_out, rhs_lo_out, 3 * (size_t)ncoef);
  for (int sp = 0; sp <= nspan; ++sp) first_out[sp] = fh_first[sp];
  *fail_out = fh;
  return MVUS_OK;
}
template <class T>
static int fit_penalty_run(int32_t device, int ncoef, int n8, const double* b, double* BtB_out, double* BtB_lo_out) {
  CallBuffers cb;
  cb.open(device);
  const double* bd = cb.put(b, 5 * (size_t)n8);
  T* BtB = cb.get<T>(5 * (size_t)ncoef);
  hipLaunchKernelGGL(k_fit_penalty<T>, fit_blocks(ncoef), dim3(256), 0, cb.st, ncoef, n8, bd, BtB);
  MVUS_HIP(hipGetLastError());
  band_read(cb, BtB, BtB_out, BtB_lo_out, 5 * (size_t)ncoef);
  return MVUS_OK;
}

extern "C" {

int mvus_spline_eval(int32_t device, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots,
                     const double* coefs, int64_t nt, const double* t, double* X, int32_t* which) {
  if (S < 1 || !interval || !knot_offsets || !knots || !coefs || nt < 0 || (nt > 0 && (!t || !X || !which))) { g_create_error = "spline_eval: bad arguments"; return MVUS_E_INVALID; }
  for (int s = 0; s < S; ++s)
    if (knot_offsets[s + 1] - knot_offsets[s] < 8) { g_create_error = "spline_eval: a cubic spline needs at least 8 knots"; return MVUS_E_INVALID; }
  if (nt == 0) return MVUS_OK;
  return stateless([&] {
    CallBuffers cb;
    cb.open(device);
    std::vector<long long> koff(knot_offsets, knot_offsets + S + 1), coff(S + 1, 0);
    for (int s = 0; s < S; ++s) coff[s + 1] = coff[s] + 3 * (koff[s + 1] - koff[s] - 4);
    SplineSet sp;
    sp.S = S;
    sp.istart = cb.put(interval, (size_t)S); sp.iend = cb.put(interval + S, (size_t)S);
    sp.knot_off = cb.put(koff.data(), koff.size()); sp.knots = cb.put(knots, (size_t)koff[S]);
    sp.coef_off = cb.put(coff.data(), coff.size()); sp.coefs = cb.put(coefs, (size_t)coff[S]);
    const double* dt = cb.put(t, (size_t)nt);
    double* dX = cb.get<double>(3 * (size_t)nt);
    int32_t* dw = cb.get<int32_t>((size_t)nt);
    hipLaunchKernelGGL(k_spline_eval, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, cb.st, sp, (long long)nt, dt, dX, dw);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(X, dX, sizeof(double) * 3 * nt, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(which, dw, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    return MVUS_OK;
  });
}

int mvus_spline_cov_eval(int32_t device, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots,
                         const double* cov_band, int64_t nt, const double* t, double* cov, int32_t* which) {
  if (S < 1 || !interval || !knot_offsets || !knots || !cov_band || nt < 0 || (nt > 0 && (!t || !cov || !which))) { g_create_error = "spline_cov_eval: bad arguments"; return MVUS_E_INVALID; }
  for (int s = 0; s < S; ++s)
    if (knot_offsets[s + 1] - knot_offsets[s] < 8) { g_create_error = "spline_cov_eval: a cubic spline needs at least 8 knots"; return MVUS_E_INVALID; }
  if (nt == 0) return MVUS_OK;
  return stateless([&] {
    CallBuffers cb;
    cb.open(device);
    std::vector<long long> koff(knot_offsets, knot_offsets + S + 1), coff(S + 1, 0);
    for (int s = 0; s < S; ++s) coff[s + 1] = coff[s] + (koff[s + 1] - koff[s] - 4);        // control points, not coefficients
    SplineSet sp;
    sp.S = S;
    sp.istart = cb.put(interval, (size_t)S); sp.iend = cb.put(interval + S, (size_t)S);
    sp.knot_off = cb.put(koff.data(), koff.size()); sp.knots = cb.put(knots, (size_t)koff[S]);
    sp.coef_off = nullptr; sp.coefs = nullptr;
    const long long* dcoff = cb.put(coff.data(), coff.size());
    const double* dband = cb.put(cov_band, (size_t)coff[S] * 36);
    const double* dt = cb.put(t, (size_t)nt);
    double* dC = cb.get<double>(9 * (size_t)nt);
    int32_t* dw = cb.get<int32_t>((size_t)nt);
    hipLaunchKernelGGL(k_spline_cov_eval, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, cb.st, sp, dcoff, dband, (long long)nt, dt, dC, dw);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(cov, dC, sizeof(double) * 9 * nt, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(which, dw, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    return MVUS_OK;
  });
}

// ---- kinematics: the three calls share mvus_spline_eval's arguments and its checks -------------------------------------------------------
static bool kin_args_ok(const char* name, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots, const void* values, int64_t nt,
                        const double* t, const void* out, const int32_t* which) {
  if (S < 1 || !interval || !knot_offsets || !knots || !values || nt < 0 || (nt > 0 && (!t || !out || !which))) { g_create_error = std::string(name) + ": bad arguments"; return false; }
  for (int s = 0; s < S; ++s)
    if (knot_offsets[s + 1] - knot_offsets[s] < 8) { g_create_error = std::string(name) + ": a cubic spline needs at least 8 knots"; return false; }
  return true;
}
// the splines on the device (coefs may be NULL: no coefficients uploaded); ctrl[s] receives the number of control points before spline s
static SplineSet kin_upload(CallBuffers& cb, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots, const double* coefs,
                            std::vector<long long>& ctrl) {
  std::vector<long long> koff(knot_offsets, knot_offsets + S + 1), coff(S + 1, 0);
  ctrl.assign(S + 1, 0);
  for (int s = 0; s < S; ++s) { ctrl[s + 1] = ctrl[s] + (koff[s + 1] - koff[s] - 4); coff[s + 1] = 3 * ctrl[s + 1]; }
  SplineSet sp;
  sp.S = S;
  sp.istart = cb.put(interval, (size_t)S); sp.iend = cb.put(interval + S, (size_t)S);
  sp.knot_off = cb.put(koff.data(), koff.size()); sp.knots = cb.put(knots, (size_t)koff[S]);
  sp.coef_off = coefs ? cb.put(coff.data(), coff.size()) : nullptr;
  sp.coefs = coefs ? cb.put(coefs, (size_t)coff[S]) : nullptr;
  return sp;
}

int mvus_spline_eval_der(int32_t device, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots,
                         const double* coefs, int64_t nt, const double* t, int32_t nder, double* D, int32_t* which) {
  if (!kin_args_ok("spline_eval_der", S, interval, knot_offsets, knots, coefs, nt, t, D, which)) return MVUS_E_INVALID;
  if (nder < 0 || nder > 2) { g_create_error = "spline_eval_der: nder must be 0, 1 or 2"; return MVUS_E_INVALID; }
  if (nt == 0) return MVUS_OK;
  return stateless([&] {
    CallBuffers cb;
    cb.open(device);
    std::vector<long long> ctrl;
    const SplineSet sp = kin_upload(cb, S, interval, knot_offsets, knots, coefs, ctrl);
    const size_t rows = 3 * (size_t)(nder + 1);
    const double* dt = cb.put(t, (size_t)nt);
    double* dD = cb.get<double>(rows * (size_t)nt);
    int32_t* dw = cb.get<int32_t>((size_t)nt);
    hipLaunchKernelGGL(k_spline_eval_der, fit_blocks(nt), dim3(256), 0, cb.st, sp, (long long)nt, dt, (int)nder, dD, dw);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(D, dD, sizeof(double) * rows * nt, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(which, dw, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    return MVUS_OK;
  });
}

int mvus_spline_kin_cov_eval(int32_t device, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots,
                             const double* cov_band, int64_t nt, const double* t, int32_t nder, double* cov, int32_t* which) {
  if (!kin_args_ok("spline_kin_cov_eval", S, interval, knot_offsets, knots, cov_band, nt, t, cov, which)) return MVUS_E_INVALID;
  if (nder < 0 || nder > 2) { g_create_error = "spline_kin_cov_eval: nder must be 0, 1 or 2"; return MVUS_E_INVALID; }
  if (nt == 0) return MVUS_OK;
  return stateless([&] {
    CallBuffers cb;
    cb.open(device);
    std::vector<long long> ctrl;
    const SplineSet sp = kin_upload(cb, S, interval, knot_offsets, knots, nullptr, ctrl);
    const long long* dctrl = cb.put(ctrl.data(), ctrl.size());
    const double* dband = cb.put(cov_band, (size_t)ctrl[S] * 36);
    const size_t dd = (size_t)kin_dim(nder) * kin_dim(nder);
    const double* dt = cb.put(t, (size_t)nt);
    double* dC = cb.get<double>(dd * (size_t)nt);
    int32_t* dw = cb.get<int32_t>((size_t)nt);
    if (nder == 0) hipLaunchKernelGGL(k_spline_kin_cov_eval<0>, fit_blocks(nt), dim3(256), 0, cb.st, sp, dctrl, dband, (long long)nt, dt, dC, dw);
    else if (nder == 1) hipLaunchKernelGGL(k_spline_kin_cov_eval<1>, fit_blocks(nt), dim3(256), 0, cb.st, sp, dctrl, dband, (long long)nt, dt, dC, dw);
    else hipLaunchKernelGGL(k_spline_kin_cov_eval<2>, fit_blocks(nt), dim3(256), 0, cb.st, sp, dctrl, dband, (long long)nt, dt, dC, dw);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(cov, dC, sizeof(double) * dd * nt, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(which, dw, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    return MVUS_OK;
  });
}

int mvus_spline_length(int32_t device, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots,
                       const double* coefs, int64_t nt, const double* t, double* dist, int32_t* which, double* total) {
  if (!kin_args_ok("spline_length", S, interval, knot_offsets, knots, coefs, nt, t, dist, which)) return MVUS_E_INVALID;
  if (nt == 0 && !total) return MVUS_OK;
  return stateless([&] {
    CallBuffers cb;
    cb.open(device);
    std::vector<long long> ctrl;
    const SplineSet sp = kin_upload(cb, S, interval, knot_offsets, knots, coefs, ctrl);
    std::vector<long long> soff(S + 1, 0);                                 // spans (l = 3 .. n - 1) before spline s
    for (int s = 0; s < S; ++s) soff[s + 1] = soff[s] + (ctrl[s + 1] - ctrl[s] - 3);
    const long long* dsoff = cb.put(soff.data(), soff.size());
    double* dlen = cb.get<double>((size_t)soff[S]);
    double* dtot = cb.get<double>((size_t)S);
    hipLaunchKernelGGL(k_span_length, fit_blocks(soff[S]), dim3(256), 0, cb.st, sp, dsoff, dlen);
    hipLaunchKernelGGL(k_span_prefix, dim3((unsigned)S), dim3(64), 0, cb.st, (int)S, dsoff, dlen, dtot);
    MVUS_HIP(hipGetLastError());
    if (nt > 0) {
      const double* dt = cb.put(t, (size_t)nt);
      double* dd = cb.get<double>((size_t)nt);
      int32_t* dw = cb.get<int32_t>((size_t)nt);
      hipLaunchKernelGGL(k_spline_length, fit_blocks(nt), dim3(256), 0, cb.st, sp, dsoff, dlen, (long long)nt, dt, dd, dw);
      MVUS_HIP(hipGetLastError());
      MVUS_HIP(hipMemcpyAsync(dist, dd, sizeof(double) * nt, hipMemcpyDeviceToHost, cb.st));
      MVUS_HIP(hipMemcpyAsync(which, dw, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, cb.st));
    }
    if (total) MVUS_HIP(hipMemcpyAsync(total, dtot, sizeof(double) * S, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    return MVUS_OK;
  });
}

int mvus_spline_lsq(int32_t device, int32_t num_knots, const double* knots, int64_t m, const double* t, const double* X, double* coefs) {
  const int n = num_knots - 4;
  if (num_knots < 8 || !knots || m < 1 || !t || !X || !coefs) { g_create_error = "spline_lsq: bad arguments"; return MVUS_E_INVALID; }
  for (int k = 1; k < num_knots; ++k) if (knots[k] < knots[k - 1]) { g_create_error = "spline_lsq: knot vector must be non-decreasing"; return MVUS_E_INVALID; }
  for (int64_t i = 0; i < m; ++i) if (!(t[i] >= knots[3] && t[i] <= knots[n])) { g_create_error = "spline_lsq: data outside the knot interval"; return MVUS_E_INVALID; }
  if (m < n) { g_create_error = "spline_lsq: fewer samples than coefficients (Schoenberg-Whitney violated)"; return MVUS_E_NUMERIC; }
  return stateless([&] {
    CallBuffers cb;
    cb.open(device);
    const double* dk = cb.put(knots, (size_t)num_knots);
    const double* dt = cb.put(t, (size_t)m);
    const double* dX = cb.put(X, 3 * (size_t)m);
    double* G = cb.get<double>(4 * (size_t)n);
    double* rhs = cb.get<double>(3 * (size_t)n);
    int* fail = cb.get<int>(1);
    MVUS_HIP(hipMemsetAsync(G, 0, sizeof(double) * 4 * n, cb.st));
    MVUS_HIP(hipMemsetAsync(rhs, 0, sizeof(double) * 3 * n, cb.st));
    MVUS_HIP(hipMemsetAsync(fail, 0, sizeof(int), cb.st));
    hipLaunchKernelGGL(k_lsq_accumulate, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, cb.st, dk, n, (long long)m, dt, dX, G, rhs);
    hipLaunchKernelGGL(k_lsq_solve, dim3(1), dim3(64), 0, cb.st, n, G, rhs, fail);
    MVUS_HIP(hipGetLastError());
    int fh = 0;
    MVUS_HIP(hipMemcpyAsync(coefs, rhs, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(&fh, fail, sizeof(int), hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    if (fh) { g_create_error = "spline_lsq: the normal equations are not positive definite to working precision (the data do not determine every coefficient: Schoenberg-Whitney violated)"; return MVUS_E_NUMERIC; }
    return MVUS_OK;
  });
}

/* scipy.interpolate.splprep(X, w=w, u=u, s=s, k=3) on the GPU (spline_fit.hip.h): fppara's control flow here, every pass over the
 * samples and every banded solve on the device.  A SESSION holds the samples (checked and uploaded once) and the work arrays:
 * traj_to_spline's smooth_factor loop fits the same samples a dozen times with different s. */
struct mvus_spline_fit {
  CallBuffers cb;
  int64_t m = 0;
  std::vector<double> hu;                                  // the timestamps on the host (fpknot places knots at samples)
  const double *du = nullptr, *dX = nullptr, *dw = nullptr;      // dw: the weights of a weighted session, else NULL
  dd* bb = nullptr;                                        // weighted session: |w x|^2 on the device (k_fit_wx2), summed when first needed
  bool bb_ready = false;
  double* fp_factor = nullptr;                             // ... and where that kernel leaves f_p
  int32_t* span = nullptr;
  double *q = nullptr, *term = nullptr, *tot_part = nullptr, *fp_part = nullptr;
  int* fail = nullptr;
  long long* first = nullptr;
  double *cd = nullptr, *td = nullptr, *bd = nullptr, *out = nullptr;
  FitWork<double> w1;
  FitWork<dd> w2;
  size_t cap = 0;
};
static int spline_fit_open_impl(mvus_spline_fit& S, int32_t device, int64_t m, const double* u, const double* X, const double* w) {
  constexpr int k = 3;
  if (m <= k || m > (1ll << 30) || !u || !X) { g_create_error = "spline_smooth: bad arguments (m > 3 samples, s > 0)"; return MVUS_E_INVALID; }
  for (int64_t i = 1; i < m; ++i) if (!(u[i] > u[i - 1])) { g_create_error = "spline_smooth: the timestamps must be strictly increasing"; return MVUS_E_INVALID; }
  for (int64_t i = 0; i < 3 * m; ++i) if (!std::isfinite(X[i])) { g_create_error = "spline_smooth: non-finite sample"; return MVUS_E_INVALID; }
  if (!fit_weights_ok(m, w)) { g_create_error = std::string("spline_smooth: ") + kFitWeightsWrong; return MVUS_E_INVALID; }
  return stateless([&] {
    S.m = m;
    S.hu.assign(u, u + m);
    CallBuffers& cb = S.cb;
    cb.open(device);
    S.du = cb.put(u, (size_t)m);
    S.dX = cb.put(X, 3 * (size_t)m);
    if (w) {
      S.dw = cb.put(w, (size_t)m);
      S.fp_factor = cb.get<double>(1);
      S.bb = cb.get<dd>(1);
    }
    S.span = cb.get<int32_t>((size_t)m);
    S.q = cb.get<double>(4 * (size_t)m);
    S.term = cb.get<double>((size_t)m);
    S.tot_part = cb.get<double>(kFitTotalParts);
    S.fp_part = cb.get<double>(512 + kFitSliceBlocks);
    S.fail = cb.get<int>(1);
    MVUS_HIP(hipStreamSynchronize(cb.st));                 // u, X and w may go away after this call
    return MVUS_OK;
  });
}
static int spline_fit_run(mvus_spline_fit& S, double s, int32_t* n_out, double* t_out, double* c_out, double* fp_out, int32_t* ier_out) {
  constexpr int k = 3, k1 = 4, k2 = 5, nmin = 8, maxit = 20;
  constexpr double tol = 0.001;
  const int64_t m = S.m;
  const double* u = S.hu.data();
  if (!n_out || !t_out || !c_out || !(s > 0.0) || !std::isfinite(s)) { g_create_error = "spline_smooth: bad arguments (m > 3 samples, s > 0)"; return MVUS_E_INVALID; }
  const bool timing = std::getenv("MVUS_FIT_TIMING") != nullptr;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const auto t_begin = now();
  int passes = 0;
  const int nest = (int)m + 2 * k, nmax = (int)m + k1;
  const auto t_checked = now();
  auto t_ready = t_checked, t_fitted = t_checked;
  const int rc = stateless([&] {
    CallBuffers& cb = S.cb;
    const double* du = S.du;
    const double* dX = S.dX;
    const double* dw = S.dw;
    int32_t* span = S.span;
    double* q = S.q;
    double* term = S.term;
    double* tot_part = S.tot_part;
    double* fp_part = S.fp_part;
    // Everything indexed by knots is sized by a CAPACITY that grows with the knot count (x4, up to FITPACK's nest = m + 6), not
    // by nest: the trajectories traj_to_spline fits are 50x oversampled (560k samples for ~600 knots), and allocating and
    // freeing ~40 arrays of nest doubles (430 MB with the double-double set) cost 70 of the 77 ms of such a fit
    long long*& first = S.first;
    double *&cd = S.cd, *&td = S.td, *&bd = S.bd, *&out = S.out;          // out: [0] sum diag(L), [1] f_p, [2] min diag(L), [3] max diag(L), [4..] residual per span
    int* fail = S.fail;
    FitWork<double>& w1 = S.w1;
    FitWork<dd>& w2 = S.w2;
    w1.penalty = false; w2.penalty = false;              // (the work arrays outlive a fit; what they hold does not)
    bool precise = false;                                  // double-double from the first ill-conditioned pass on
    bool diag_natural = true;                              // out[0] of the last least-squares pass is the sum FITPACK forms (see fit_band_solve)
    int lsq_dd_n = -1;                                     // knot count whose normal equations w2 holds
    bool fp_from_factor = false;                           // the last least-squares pass left its f_p in S.fp_factor (k_fit_fp_from_factor)
    MVUS_HIP(hipMemsetAsync(fail, 0, sizeof(int), cb.st));
    std::vector<double> t, fpint, host, b;
    std::vector<int> nrdata;
    size_t& cap = S.cap;
    auto ensure = [&](size_t need) {                      // between passes only: the device arrays hold nothing that outlives a pass
      if (need <= cap || cap >= (size_t)nest) return;     // (nest = m + 6 knots is all FITPACK can ever ask for: nothing to grow to)
      size_t c = std::max<size_t>(cap, 1024);
      while (c < need) c *= 4;
      cap = std::min<size_t>(c, (size_t)nest);
      first = cb.get<long long>(cap + 1); cd = cb.get<double>(3 * cap); td = cb.get<double>(cap); bd = cb.get<double>(5 * cap);
      out = cb.get<double>(cap + 4);
      w1 = FitWork<double>(); w2 = FitWork<dd>(); lsq_dd_n = -1;
      w1.alloc(cb, cap);
      if (t.size() < cap) { t.resize(cap, 0.0); fpint.resize(cap, 0.0); nrdata.resize(cap, 0); }
      if (host.size() < cap + 4) host.resize(cap + 4, 0.0);
    };
    ensure(nmin + 16);
    if (t.size() < cap) { t.resize(cap, 0.0); fpint.resize(cap, 0.0); nrdata.resize(cap, 0); }      // (capacity kept from an earlier fit of this session)
    if (host.size() < cap + 4) host.resize(cap + 4, 0.0);
    if (timing) { MVUS_HIP(hipStreamSynchronize(cb.st)); t_ready = now(); }
    const double ub = u[0], ue = u[m - 1], acc = tol * s;
    int n = nmin, nplus = 0, ier = 0, nrint = 1, failed = 0;
    double fpold = 0.0, fp0 = 0.0, fp = 0.0, p = -1.0;
    nrdata[0] = (int)m - 2;
    auto blocks = fit_blocks;
    auto residual = [&](int ncoef, bool spans, int nspan) {            // c -> f_p (and the per-span residuals), fetched
      fit_residual_pass(cb.st, (long long)m, ncoef, span, q, dX, dw, cd, term, tot_part, out, spans, nspan, fit_slices(nspan), first, fp_part);
      MVUS_HIP(hipGetLastError());
      MVUS_HIP(hipMemcpyAsync(host.data(), out, sizeof(double) * (4 + (spans ? nspan : 0)), hipMemcpyDeviceToHost, cb.st));
      MVUS_HIP(hipMemcpyAsync(&failed, fail, sizeof(int), hipMemcpyDeviceToHost, cb.st));
      MVUS_HIP(hipStreamSynchronize(cb.st));
    };
    // a pass in fp64; when its Cholesky breaks down or the factor's diagonal spans more than four decades (cond(A^T A) >= 1e8)
    // the pass is repeated in double-double, and so is every later pass of this call
    auto ill = [&] { return failed != 0 || !(host[3] <= 1e4 * host[2]); };
    auto solve = [&](int ncoef, int nrint_, int n8, bool smoothing, double pinv) {
      for (int attempt = 0; attempt < 2; ++attempt) {
        if (!precise) {
          if (!smoothing) diag_natural = fit_lsq_pass<double>(cb.st, w1, (long long)m, first, q, dX, dw, ncoef, nrint_, fit_slices(nrint_), band_parts(ncoef, 3, band_parts_min()), cd, out, fail);
          else fit_smooth_pass<double>(cb.st, w1, ncoef, n8, bd, pinv, cd, out, fail);
        } else {
          w2.alloc(cb, cap);
          if (lsq_dd_n != n) {
            // A weighted fit close to interpolation (the rule at the call of solve below): f_p from the factorisation, for which the
            // system is solved in ONE chain -- its forward substitution is what k_fit_fp_from_factor reads.  A chain costs 4.8 us a row in
            // double-double where the partitioned solver takes a fraction of that; at most m / 2 ... m + 2 rows here, and only here: a
            // weighted pass that is in double-double through the test on the pivots keeps the partition and the residual's own sum.
            fp_from_factor = dw && 2ll * ncoef > m;
            diag_natural = fit_lsq_pass<dd>(cb.st, w2, (long long)m, first, q, dX, dw, ncoef, nrint_, fit_slices(nrint_),
                                            fp_from_factor ? BandParts() : band_parts(ncoef, 3, band_parts_min()), cd, out, fail);
            if (fp_from_factor && !S.bb_ready) { hipLaunchKernelGGL(k_fit_wx2, dim3(1), dim3(256), 0, cb.st, (long long)m, dX, dw, S.bb); S.bb_ready = true; }
            if (fp_from_factor) hipLaunchKernelGGL(k_fit_fp_from_factor, dim3(1), dim3(256), 0, cb.st, 3 * ncoef, w2.yw, S.bb, S.fp_factor);
            lsq_dd_n = n;
          }
          if (smoothing) fit_smooth_pass<dd>(cb.st, w2, ncoef, n8, bd, pinv, cd, out, fail);
        }
        residual(ncoef, !smoothing, nrint_);
        if (precise && fp_from_factor && !smoothing && !failed) {      // f_p of this pass from its factorisation (no floored pivot in it)
          MVUS_HIP(hipMemcpyAsync(&host[1], S.fp_factor, sizeof(double), hipMemcpyDeviceToHost, cb.st));
          MVUS_HIP(hipStreamSynchronize(cb.st));
        }
        ++passes;
        if (std::getenv("MVUS_DEBUG")) std::fprintf(stderr, "spline_smooth: n=%d %s %s  diag(L) %.3e..%.3e  fp %.6e  fail %d\n", n, smoothing ? "smooth" : "lsq",
                                                    precise ? "dd" : "fp64", host[2], host[3], host[1], failed);
        if (precise) {                                    // floored pivots are accepted here (see k_band_solve)
          if (!std::isfinite(host[1])) throw HipError{"spline_smooth: a banded system is not positive definite", MVUS_E_NUMERIC};
          MVUS_HIP(hipMemsetAsync(fail, 0, sizeof(int), cb.st));
          return;
        }
        if (!ill()) return;
        precise = true;
        MVUS_HIP(hipMemsetAsync(fail, 0, sizeof(int), cb.st));
      }
    };
    int ncoef = 0;
    for (;;) {                                             // fppara: do 200 iter = 1, m
      ensure((size_t)n + 16);
      if (n == nmin) ier = -2;
      nrint = n - nmin + 1;
      ncoef = n - k1;
      for (int j = 0; j < k1; ++j) { t[j] = ub; t[n - 1 - j] = ue; }
      MVUS_HIP(hipMemcpyAsync(td, t.data(), sizeof(double) * n, hipMemcpyHostToDevice, cb.st));
      MVUS_HIP(hipStreamSynchronize(cb.st));               // t is modified on the host below
      hipLaunchKernelGGL(k_fit_basis, blocks(m), dim3(256), 0, cb.st, (long long)m, du, td, ncoef, span, q);
      hipLaunchKernelGGL(k_fit_first, blocks(nrint + 1), dim3(256), 0, cb.st, (long long)m, du, td, nrint, first);
      // A weighted fit goes to double-double once it has more than half as many coefficients as samples.  Close to interpolation a knot
      // set can be rank deficient to fp64 (cond(A) 5e15 at 313 coefficients for 349 samples in tests/test_gpu_weighted_fit.py, seed 6)
      // through the growth of the back substitution along a run of one-sample spans, with every Cholesky pivot of ordinary size: the test
      // on the factor's diagonal below does not see it, the residuals are off by 5 % and the knot search leaves FITPACK's path.  Weights
      // enter the normal equations squared and use up the margin the unweighted fit has there; that fit keeps its own rule and its bits.
      if (dw && !precise && 2ll * ncoef > m) precise = true;
      solve(ncoef, nrint, 0, false, 0.0);
      fp = host[1];
      if (ier == -2) fp0 = fp;
      double fpms = fp - s;
      if (std::fabs(fpms) < acc) break;
      if (fpms < 0.0) {
        if (ier == -2) break;                              // the least-squares polynomial is acceptable
        // ---- part 2: the smoothing spline, F(p) = s ----
        fitpack::fpdisc(t, n, b);
        const int n8 = n - nmin;
        MVUS_HIP(hipMemcpyAsync(bd, b.data(), sizeof(double) * b.size(), hipMemcpyHostToDevice, cb.st));
        double p1 = 0.0, f1 = fp0 - s, p3 = -1.0, f3 = fpms;
        if (!diag_natural) {                               // the pass above was partitioned: one chain over the same normal equations for sum a(i,1)
          if (precise) fit_lsq_diag<dd>(cb.st, w2, ncoef, out); else fit_lsq_diag<double>(cb.st, w1, ncoef, out);
          MVUS_HIP(hipGetLastError());
          MVUS_HIP(hipMemcpyAsync(host.data(), out, sizeof(double), hipMemcpyDeviceToHost, cb.st));
          MVUS_HIP(hipStreamSynchronize(cb.st));
        }
        p = (double)ncoef / host[0];
        int ich1 = 0, ich3 = 0;
        for (int iter = 1; iter <= maxit; ++iter) {
          solve(ncoef, nrint, n8, true, 1.0 / p);
          fp = host[1];
          fpms = fp - s;
          if (std::fabs(fpms) < acc) break;
          if (iter == maxit) { ier = 3; break; }
          const double p2 = p, f2 = fpms;
          if (ich3 == 0) {
            if (f2 - f3 <= acc) {                          // the initial choice of p is too large
              p3 = p2; f3 = f2;
              p = p * 0.04;
              if (p <= p1) p = p1 * 0.9 + p2 * 0.1;
              continue;
            }
            if (f2 < 0.0) ich3 = 1;
          }
          if (ich1 == 0) {
            if (f1 - f2 <= acc) {                          // the initial choice of p is too small
              p1 = p2; f1 = f2;
              p = p / 0.04;
              if (p3 < 0.0) continue;
              if (p >= p3) p = p2 * 0.1 + p3 * 0.9;
              continue;
            }
            if (f2 > 0.0) ich1 = 1;
          }
          if (f2 >= f1 || f2 <= f3) { ier = 2; break; }
          p = fitpack::fprati(p1, f1, p2, f2, p3, f3);
        }
        if (ier < 0) ier = 0;
        break;
      }
      if (n == nmax) { ier = -1; break; }
      if (n == nest) { ier = 1; break; }
      // ---- more knots ----
      if (ier == 0) {
        int npl1 = nplus * 2;
        const double rn = nplus;
        if (fpold - fp > acc) npl1 = (int)(rn * fpms / (fpold - fp));
        nplus = std::min(nplus * 2, std::max(std::max(npl1, nplus / 2), 1));
      } else {
        nplus = 1;
        ier = 0;
      }
      fpold = fp;
      {                                                    // room for the knots about to be added (host arrays; the device side follows at the top of the loop)
        const size_t need = std::min<size_t>((size_t)nest, (size_t)n + (size_t)nplus + 16);
        if (need > t.size()) { t.resize(need, 0.0); fpint.resize(need, 0.0); nrdata.resize(need, 0); }
      }
      for (int j = 0; j < nrint; ++j) fpint[j] = host[4 + j];
      fitpack::fpknot_batch(u, t, n, fpint, nrdata, nrint, nplus, nmax, nest);
      if (n == nmax) {                                      // fppara label 10: the knots of the interpolating spline
        if (t.size() < (size_t)nest) { t.resize((size_t)nest, 0.0); fpint.resize((size_t)nest, 0.0); nrdata.resize((size_t)nest, 0); }
        int i = k2, j = k / 2 + 2;
        for (int l = 0; l < (int)m - k1; ++l) { t[i - 1] = u[j - 1]; ++i; ++j; }
      }
    }
    t_fitted = now();
    std::vector<double> ch(3 * (size_t)ncoef);
    MVUS_HIP(hipMemcpyAsync(ch.data(), cd, sizeof(double) * 3 * ncoef, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    for (int d = 0; d < 3; ++d) for (int j = 0; j < ncoef; ++j) c_out[(size_t)d * nest + j] = ch[(size_t)d * ncoef + j];
    for (int j = 0; j < n; ++j) t_out[j] = t[j];
    *n_out = n;
    if (fp_out) *fp_out = fp;
    if (ier_out) *ier_out = ier;
    if (timing) std::fprintf(stderr, "spline_smooth: m=%lld n=%d passes=%d | input checks %.2f ms, buffers+upload %.2f ms, passes %.2f ms", (long long)m, n, passes,
                             ms(t_begin, t_checked), ms(t_checked, t_ready), ms(t_ready, t_fitted));
    return MVUS_OK;
  });
  if (rc == MVUS_OK && timing) std::fprintf(stderr, ", total %.2f ms\n", ms(t_begin, now()));
  return rc;
}

int mvus_spline_fit_open_w(int32_t device, int64_t m, const double* u, const double* X, const double* w, mvus_spline_fit** out) {
  if (!out) { g_create_error = "spline_fit_open: bad arguments"; return MVUS_E_INVALID; }
  *out = nullptr;
  mvus_spline_fit* S = nullptr;
  try { S = new mvus_spline_fit(); } catch (const std::exception& e) { g_create_error = e.what(); return MVUS_E_INVALID; }
  const int rc = spline_fit_open_impl(*S, device, m, u, X, w);
  if (rc != MVUS_OK) { delete S; return rc; }
  *out = S;
  return MVUS_OK;
}
int mvus_spline_fit_open(int32_t device, int64_t m, const double* u, const double* X, mvus_spline_fit** out) {
  return mvus_spline_fit_open_w(device, m, u, X, nullptr, out);
}
int mvus_spline_fit_smooth(mvus_spline_fit* S, double s, int32_t* n_out, double* t_out, double* c_out, double* fp_out, int32_t* ier_out) {
  if (!S) { g_create_error = "spline_fit_smooth: no session"; return MVUS_E_INVALID; }
  return spline_fit_run(*S, s, n_out, t_out, c_out, fp_out, ier_out);
}
void mvus_spline_fit_close(mvus_spline_fit* S) { delete S; }

int mvus_spline_smooth_w(int32_t device, int64_t m, const double* u, const double* X, const double* w, double s, int32_t* n_out, double* t_out,
                         double* c_out, double* fp_out, int32_t* ier_out) {
  if (!n_out || !t_out || !c_out || !(s > 0.0) || !std::isfinite(s)) { g_create_error = "spline_smooth: bad arguments (m > 3 samples, s > 0)"; return MVUS_E_INVALID; }
  mvus_spline_fit S;
  const int rc = spline_fit_open_impl(S, device, m, u, X, w);
  if (rc != MVUS_OK) return rc;
  return spline_fit_run(S, s, n_out, t_out, c_out, fp_out, ier_out);
}
int mvus_spline_smooth(int32_t device, int64_t m, const double* u, const double* X, double s, int32_t* n_out, double* t_out, double* c_out,
                       double* fp_out, int32_t* ier_out) {
  return mvus_spline_smooth_w(device, m, u, X, nullptr, s, n_out, t_out, c_out, fp_out, ier_out);
}

int mvus_spline_band_solve(int32_t device, int32_t n, int32_t hb, int32_t precise, int32_t parts, const double* G5, const double* G5_lo, const double* BtB,
                           const double* BtB_lo, double pinv, const double* rhs, const double* rhs_lo, double* c_out, double* stats_out, int32_t* fail_out,
                           int32_t* P_out) {
  if (n < 4 || (hb != 3 && hb != 4) || !G5 || !rhs || !c_out || !stats_out || !fail_out || !P_out) { g_create_error = "spline_band_solve: bad arguments (n >= 4, hb 3 or 4)"; return MVUS_E_INVALID; }
  if (hb == 3 && (BtB || BtB_lo)) { g_create_error = "spline_band_solve: hb = 3 solves G5 alone, BtB must be NULL"; return MVUS_E_INVALID; }
  if (hb == 4 && (!BtB || !std::isfinite(pinv))) { g_create_error = "spline_band_solve: hb = 4 needs BtB and a finite pinv"; return MVUS_E_INVALID; }
  if (parts < -1 || parts == 1 || (parts >= 2 && !band_parts_legal(n, hb, parts))) {
    g_create_error = "spline_band_solve: parts must be -1 (one chain), 0 (the production rule) or 2..256 interiors of at least 2 hb rows";
    return MVUS_E_INVALID;
  }
  BandParts bp;
  bp.HB = hb;
  if (parts == 0) bp = band_parts(n, hb, 192);
  else if (parts >= 2) bp = band_parts_fixed(n, hb, parts);
  *P_out = bp.P;
  return stateless([&] {
    return precise ? band_solve_run<dd>(device, n, hb, bp, G5, G5_lo, BtB, BtB_lo, pinv, rhs, rhs_lo, c_out, stats_out, fail_out)
                   : band_solve_run<double>(device, n, hb, bp, G5, G5_lo, BtB, BtB_lo, pinv, rhs, rhs_lo, c_out, stats_out, fail_out);
  });
}

int mvus_spline_band_diag_sum(int32_t device, int32_t n, int32_t precise, const double* G5, const double* G5_lo, double* out) {
  if (n < 4 || !G5 || !out) { g_create_error = "spline_band_diag_sum: bad arguments (n >= 4)"; return MVUS_E_INVALID; }
  return stateless([&] { return precise ? band_diag_sum_run<dd>(device, n, G5, G5_lo, out) : band_diag_sum_run<double>(device, n, G5, G5_lo, out); });
}

int mvus_spline_fit_normal_w(int32_t device, int64_t m, const double* u, const double* X, const double* w, int32_t n, const double* t, int32_t precise,
                             int32_t slices, int32_t parts, int32_t* span_out, double* q_out, int64_t* first_out, double* G5_out, double* G5_lo_out,
                             double* rhs_out, double* rhs_lo_out, double* c_out, double* stats_out, int32_t* fail_out) {
  if (!X || !span_out || !q_out || !first_out || !G5_out || !rhs_out || !c_out || !stats_out || !fail_out) { g_create_error = "spline_fit_normal: bad arguments"; return MVUS_E_INVALID; }
  if (!fit_inspect_args_ok("spline_fit_normal", m, u, X, w, n, t, slices)) return MVUS_E_INVALID;
  const int ncoef = n - 4;
  if (parts < -1 || parts == 1 || (parts >= 2 && !band_parts_legal(ncoef, 3, parts))) {
    g_create_error = "spline_fit_normal: parts must be -1 (one chain), 0 (the production rule) or 2..256 interiors of at least 6 rows";
    return MVUS_E_INVALID;
  }
  BandParts bp;
  if (parts == 0) bp = band_parts(ncoef, 3, 192);
  else if (parts >= 2) bp = band_parts_fixed(ncoef, 3, parts);
  return stateless([&] {
    return precise ? fit_normal_run<dd>(device, m, u, X, w, n, t, slices, bp, span_out, q_out, first_out, G5_out, G5_lo_out, rhs_out, rhs_lo_out, c_out, stats_out, fail_out)
                   : fit_normal_run<double>(device, m, u, X, w, n, t, slices, bp, span_out, q_out, first_out, G5_out, G5_lo_out, rhs_out, rhs_lo_out, c_out, stats_out, fail_out);
  });
}
int mvus_spline_fit_normal(int32_t device, int64_t m, const double* u, const double* X, int32_t n, const double* t, int32_t precise, int32_t slices,
                           int32_t parts, int32_t* span_out, double* q_out, int64_t* first_out, double* G5_out, double* G5_lo_out, double* rhs_out,
                           double* rhs_lo_out, double* c_out, double* stats_out, int32_t* fail_out) {
  return mvus_spline_fit_normal_w(device, m, u, X, nullptr, n, t, precise, slices, parts, span_out, q_out, first_out, G5_out, G5_lo_out, rhs_out, rhs_lo_out,
                                  c_out, stats_out, fail_out);
}

int mvus_spline_fit_penalty(int32_t device, int32_t ncoef, int32_t n8, const double* b, int32_t precise, double* BtB_out, double* BtB_lo_out) {
  if (ncoef < 5 || n8 < 1 || n8 > ncoef - 4 || !b || !BtB_out) { g_create_error = "spline_fit_penalty: bad arguments (1 <= n8 <= ncoef - 4 rows of b)"; return MVUS_E_INVALID; }
  for (int64_t i = 0; i < 5ll * n8; ++i) if (!std::isfinite(b[i])) { g_create_error = "spline_fit_penalty: non-finite b"; return MVUS_E_INVALID; }
  return stateless([&] { return precise ? fit_penalty_run<dd>(device, ncoef, n8, b, BtB_out, BtB_lo_out) : fit_penalty_run<double>(device, ncoef, n8, b, BtB_out, BtB_lo_out); });
}

int mvus_spline_fit_residual_w(int32_t device, int64_t m, const double* u, const double* X, const double* w, int32_t n, const double* t, const double* c,
                               int32_t slices, double* term_out, double* fp_out, double* fpint_out) {
  if (!X || !c || !term_out || !fp_out || !fpint_out) { g_create_error = "spline_fit_residual: bad arguments"; return MVUS_E_INVALID; }
  if (!fit_inspect_args_ok("spline_fit_residual", m, u, X, w, n, t, slices)) return MVUS_E_INVALID;
  const int ncoef = n - 4, nspan = n - 7;
  for (int i = 0; i < 3 * ncoef; ++i) if (!std::isfinite(c[i])) { g_create_error = "spline_fit_residual: non-finite coefficient"; return MVUS_E_INVALID; }
  return stateless([&] {
    CallBuffers cb;
    cb.open(device);
    FitInputs in;
    in.upload(cb, m, u, X, w, n, t);
    const double* cd = cb.put(c, 3 * (size_t)ncoef);
    double* term = cb.get<double>((size_t)m);
    double* tot_part = cb.get<double>(kFitTotalParts);
    double* fp_part = cb.get<double>(512 + kFitSliceBlocks);
    double* out = cb.get<double>((size_t)n + 4);
    fit_residual_pass(cb.st, (long long)m, ncoef, in.span, in.q, in.dX, in.dw, cd, term, tot_part, out, true, nspan, slices ? slices : fit_slices(nspan), in.first, fp_part);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(term_out, term, sizeof(double) * m, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(fp_out, out + 1, sizeof(double), hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipMemcpyAsync(fpint_out, out + 4, sizeof(double) * nspan, hipMemcpyDeviceToHost, cb.st));
    MVUS_HIP(hipStreamSynchronize(cb.st));
    return MVUS_OK;
  });
}
int mvus_spline_fit_residual(int32_t device, int64_t m, const double* u, const double* X, int32_t n, const double* t, const double* c, int32_t slices,
                             double* term_out, double* fp_out, double* fpint_out) {
  return mvus_spline_fit_residual_w(device, m, u, X, nullptr, n, t, c, slices, term_out, fp_out, fpint_out);
}

}  // extern "C"
