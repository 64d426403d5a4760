// TEST-ONLY host build of the per-observation device math (mvus_amd/csrc/ba_math.h).
// Lets the CPU test-suite check the arithmetic the HIP kernels run (residual, analytic Jacobian)
// against the oracle without a GPU.  Never linked into libmvusba.so.
#include "../../mvus_amd/csrc/ba_math.h"
#include "../../mvus_amd/csrc/ba_switches.h"
#include "../../mvus_amd/csrc/triangulate.hip.h"
#include "../../mvus_amd/csrc/spline_fit.hip.h"
#include "../../mvus_amd/csrc/pnp.hip.h"
#include "../../mvus_amd/csrc/epipolar.hip.h"

using namespace mvus;

extern "C" int hostcheck_eval(int C, int calib, int undist, int rs_free, const int64_t* det_off,
                              const double* frame, const double* u_raw, const double* v_raw, const double* H,
                              const double* Kfix, const double* dfix, int S, const double* istart,
                              const double* iend, const double* knots, const int32_t* knot_off,
                              const int32_t* ctrl_off, const int32_t* xoff, const double* x, double* ex,
                              double* ey, int32_t* ctrl, double* J) {
  SplineView sp{S, istart, iend, knots, knot_off, ctrl_off, xoff};
  const int NS = num_slots(calib != 0);
  for (int c = 0; c < C; ++c) {
    CamState cam;
    load_cam_state(x, C, c, calib != 0, Kfix, dfix, H[c], cam);
    for (int64_t i = det_off[c]; i < det_off[c + 1]; ++i) {
      double uo = u_raw[i], vo = v_raw[i];
      if (!calib && undist) {
        double xn, yn;
        undistort5<false>((u_raw[i] - cam.cx) / cam.fx, (v_raw[i] - cam.cy) / cam.fy, cam.d, xn, yn, nullptr, nullptr);
        uo = cam.fx * xn + cam.cx;
        vo = cam.fy * yn + cam.cy;
      }
      double* jx = J + (2 * i) * NS;
      double* jy = J + (2 * i + 1) * NS;
      for (int k = 0; k < 2 * NS; ++k) jx[k] = 0.0;
      ObsResult r = calib ? eval_observation<true, true>(cam, sp, x, undist != 0, rs_free != 0, true, frame[i], u_raw[i], v_raw[i], uo, vo, jx, jy)
                          : eval_observation<false, true>(cam, sp, x, undist != 0, rs_free != 0, true, frame[i], u_raw[i], v_raw[i], uo, vo, jx, jy);
      ex[i] = r.ex; ey[i] = r.ey; ctrl[i] = r.ctrl;
    }
  }
  return 0;
}

// host build of the per-pair triangulation math (mvus_amd/csrc/triangulate.hip.h); x1, x2: [2][N], X: [4][N]
extern "C" int hostcheck_triangulate(long long N, const double* x1, const double* x2, const double* P1, const double* P2,
                                     double* X, double* err1, double* err2) {
  for (long long i = 0; i < N; ++i) {
    double Xh[4];
    triangulate_pair(P1, P2, x1[i], x1[N + i], x2[i], x2[N + i], Xh);
    for (int k = 0; k < 4; ++k) X[k * N + i] = Xh[k];
    if (err1) err1[i] = reprojection_distance(P1, Xh, x1[i], x1[N + i]);
    if (err2) err2[i] = reprojection_distance(P2, Xh, x2[i], x2[N + i]);
  }
  return 0;
}

// host parts of the smoothing-spline fit (mvus_amd/csrc/spline_fit.hip.h): FITPACK's scalar routines and the double-double
// arithmetic of the ill-conditioned passes
extern "C" void hostcheck_fpdisc(int n, const double* t, double* b_out) {
  std::vector<double> tv(t, t + n), b;
  fitpack::fpdisc(tv, n, b);
  for (size_t i = 0; i < b.size(); ++i) b_out[i] = b[i];
}
extern "C" double hostcheck_fprati(double* pf /* p1 f1 p2 f2 p3 f3, p1 f1 p3 f3 updated */) {
  return fitpack::fprati(pf[0], pf[1], pf[2], pf[3], pf[4], pf[5]);
}
extern "C" void hostcheck_fpknot(int nest, const double* x, int* n, double* t, double* fpint, int* nrdata, int* nrint) {
  std::vector<double> tv(t, t + nest), fv(fpint, fpint + nest);
  std::vector<int> nd(nrdata, nrdata + nest);
  fitpack::fpknot(x, tv, *n, fv, nd, *nrint);
  for (int i = 0; i < nest; ++i) { t[i] = tv[i]; fpint[i] = fv[i]; nrdata[i] = nd[i]; }
}
extern "C" void hostcheck_fpknot_batch(int nest, const double* x, int* n, double* t, double* fpint, int* nrdata, int* nrint, int nplus, int nmax) {
  std::vector<double> tv(t, t + nest), fv(fpint, fpint + nest);
  std::vector<int> nd(nrdata, nrdata + nest);
  fitpack::fpknot_batch(x, tv, *n, fv, nd, *nrint, nplus, nmax, nest);
  for (int i = 0; i < nest; ++i) { t[i] = tv[i]; fpint[i] = fv[i]; nrdata[i] = nd[i]; }
}
// op: 0 a+b, 1 a*b, 2 a/b, 3 sqrt(a), 4 exact product of the two high words;  a, b, out: (hi, lo)
extern "C" void hostcheck_dd(int op, const double* a, const double* b, double* out) {
  const dd x(a[0], a[1]), y(b[0], b[1]);
  dd r;
  switch (op) {
    case 0: r = x + y; break;
    case 1: r = x * y; break;
    case 2: r = x / y; break;
    case 3: r = num_sqrt(x); break;
    default: r = dd_two_prod(a[0], b[0]); break;
  }
  out[0] = r.hi; out[1] = r.lo;
}

// ---- the partition of the band solvers (spline_fit.hip.h: BandParts, band_parts, band_parts_fixed) ----
// P == 0: the production rule with `min_rows`; P >= 2: band_parts_fixed.  out = P, len, rem; returns 0 for an explicit P that is not legal
extern "C" int hostcheck_band_parts(int n, int HB, int P, int min_rows, int* out) {
  if (P != 0 && !band_parts_legal(n, HB, P)) return 0;
  const BandParts bp = P == 0 ? band_parts(n, HB, min_rows) : band_parts_fixed(n, HB, P);
  out[0] = bp.P; out[1] = bp.len; out[2] = bp.rem;
  return 1;
}
static BandParts band_parts_of(int HB, int P, int len, int rem) { BandParts bp; bp.HB = HB; bp.P = P; bp.len = len; bp.rem = rem; return bp; }
// first[P], length[P] and locate() of rows 0..n-1 of a partition
extern "C" void hostcheck_band_layout(int n, int HB, int P, int len, int rem, int* first, int* length, int* loc_p, int* loc_i) {
  const BandParts bp = band_parts_of(HB, P, len, rem);
  for (int p = 0; p < P; ++p) { first[p] = bp.first(p); length[p] = bp.length(p); }
  for (int j = 0; j < n; ++j) bp.locate(j, loc_p[j], loc_i[j]);
}
// at(p, i, k, K) for count index triples
extern "C" void hostcheck_band_at(int HB, int P, int len, int rem, int K, long long count, const int* p, const int* i, const int* k, long long* at) {
  const BandParts bp = band_parts_of(HB, P, len, rem);
  for (long long e = 0; e < count; ++e) at[e] = bp.at(p[e], i[e], k[e], K);
}
// Every legal explicit P of (n, HB), and the production rule (min_rows): violations counted per invariant, all 0 for a sound partition.
//   counts[0] partitions looked at; [1] rows whose locate() is not the walk interior 0, separator 0, interior 1, .. in order, or whose
//   first() / length() disagree with it; [2] partitions that do not end at row n; [3] interiors shorter than 2 HB;
//   [4] at() past K * rows for the K of an array (rows = n + kBandPartsMax; K = HB + 1, 3, HB); [5] with walk_at != 0: at() values that are
//   not the running count over (i, k, p), i.e. not injective
extern "C" void hostcheck_band_parts_sweep(int n, int HB, int min_rows, int walk_at, long long* counts) {
  for (int k = 0; k < 6; ++k) counts[k] = 0;
  const long long rows = (long long)n + kBandPartsMax;
  for (int P = 1; P <= kBandPartsMax; ++P) {
    BandParts bp;
    if (P == 1) { bp = band_parts(n, HB, min_rows); if (bp.P < 2) continue; }       // (P == 1 stands for the rule)
    else if (band_parts_legal(n, HB, P)) bp = band_parts_fixed(n, HB, P);
    else continue;
    ++counts[0];
    int p = 0, i = 0, lmax = 0;
    for (int j = 0; j < n; ++j) {
      int lp, li;
      bp.locate(j, lp, li);
      if (lp != p || li != i || bp.first(p) + i != j) ++counts[1];
      ++i;
      if (p + 1 < bp.P && i == bp.length(p) + HB) { ++p; i = 0; }
    }
    if (p != bp.P - 1 || i != bp.length(bp.P - 1)) ++counts[2];
    for (int q = 0; q < bp.P; ++q) { if (bp.length(q) < 2 * HB) ++counts[3]; lmax = std::max(lmax, bp.length(q)); }
    const int Ks[3] = {HB + 1, 3, HB};
    for (int K : Ks) {
      for (int q = 0; q < bp.P; ++q) if (bp.at(q, bp.length(q) - 1, K - 1, K) >= K * rows) ++counts[4];
      if (walk_at) {
        long long run = 0;
        for (int ii = 0; ii < lmax; ++ii) for (int k = 0; k < K; ++k) for (int q = 0; q < bp.P; ++q, ++run) if (bp.at(q, ii, k, K) != run) ++counts[5];
      }
    }
  }
}

// ---- the sizes of the fit's sliced passes and of its two-stage total (spline_fit.hip.h) ----
// out = kFitBlk, kFitSliceBlocks, kFitTotalOneStage, kFitTotalParts
extern "C" void hostcheck_fit_constants(long long* out) { out[0] = kFitBlk; out[1] = kFitSliceBlocks; out[2] = kFitTotalOneStage; out[3] = kFitTotalParts; }
extern "C" int hostcheck_fit_slices(int nspan) { return fit_slices(nspan); }
extern "C" int hostcheck_fit_slices_legal(int nspan, int slices) { return fit_slices_legal(nspan, slices) ? 1 : 0; }
extern "C" int hostcheck_fit_total_parts(long long m) { return fit_total_parts(m); }
// 0 when the inspection entry points accept these samples and knots
extern "C" int hostcheck_fit_samples_knots_wrong(long long m, const double* u, int n, const double* t) { return fit_samples_knots_wrong(m, u, n, t) ? 1 : 0; }

// host build of the PnP math (mvus_amd/csrc/pnp.hip.h)
extern "C" int hostcheck_pnp_dlt6(const double* Xs /* [6][3] */, const double* xn /* [6][2] */, double* R, double* t) {
  return pnp_dlt6(reinterpret_cast<const double (*)[3]>(Xs), reinterpret_cast<const double (*)[2]>(xn), R, t) ? 1 : 0;
}
extern "C" int hostcheck_pnp_project(const double* K, const double* d, const double* R, const double* t, const double* X, double* uv) {
  return pnp_project(K, d, R, t, X, uv[0], uv[1]) ? 1 : 0;
}
extern "C" int hostcheck_pnp_point_normal(const double* K, const double* d, const double* R, const double* t, const double* X, double u, double v, double* acc28) {
  for (int k = 0; k < 28; ++k) acc28[k] = 0.0;
  return pnp_point_normal(K, d, R, t, X, u, v, acc28) ? 1 : 0;
}
extern "C" void hostcheck_pnp_sample6(unsigned long long seed, int h, long long N, long long* idx) { pnp_sample6(seed, h, N, idx); }
extern "C" void hostcheck_rotation_to_rvec(const double* R, double* r) { rotation_to_rvec(R, r); }
// k_pnp_normalise for a pixel array: uv, xn: [2][N]; Kd = fx fy cx cy k1 k2 p1 p2 k3
extern "C" void hostcheck_undistort5(long long N, const double* uv, const double* Kd, double* xn) {
  for (long long i = 0; i < N; ++i) {
    double xo, yo;
    undistort5<false>((uv[i] - Kd[2]) / Kd[0], (uv[N + i] - Kd[3]) / Kd[1], Kd + 4, xo, yo, nullptr, nullptr);
    xn[i] = xo; xn[N + i] = yo;
  }
}
// k_pnp_score / k_pnp_mask for one pose: squared pixel error per point, -1 where the point is not in front.  X: [3][N]; uv, e2: [2][N], [N]
extern "C" void hostcheck_pnp_sqerr(long long N, const double* X, const double* uv, const double* Kd, const double* R, const double* t, double* e2) {
  for (long long i = 0; i < N; ++i) {
    const double Xi[3] = {X[i], X[N + i], X[2 * N + i]};
    double u, v;
    e2[i] = -1.0;
    if (pnp_project(Kd, Kd + 4, R, t, Xi, u, v)) { const double du = u - uv[i], dv = v - uv[N + i]; e2[i] = du * du + dv * dv; }
  }
}

// host build of the two-view math (mvus_amd/csrc/epipolar.hip.h)
extern "C" int hostcheck_fm_cubic_roots(const double* c /* c3 c2 c1 c0 */, double* r) { return fm_cubic_roots(c[0], c[1], c[2], c[3], r); }
extern "C" int hostcheck_fm_seven_point(const double* xs /* [7][4] */, double* Fs /* [3][9] */) {
  return fm_seven_point(reinterpret_cast<const double (*)[4]>(xs), reinterpret_cast<double (*)[9]>(Fs));
}
// x1, x2: [2][N]; err[N]
extern "C" void hostcheck_fm_error(long long N, const double* F, const double* x1, const double* x2, double* err) {
  for (long long i = 0; i < N; ++i) err[i] = fm_error(F, x1[i], x1[N + i], x2[i], x2[N + i]);
}

// ---- the switch table of the BA unit (ba_switches.h): the field behind an MVUS_* variable, read from the environment now ----
// bools as 0 / 1; -2 for a name the table does not have
extern "C" long long hostcheck_switch(const char* name) {
  const Switches s = read_switches();
  const struct { const char* name; long long value; } fields[] = {
      {"MVUS_LM_NO_CARRY", s.lm_no_carry}, {"MVUS_FETCH_EVENT", s.fetch_event}, {"MVUS_NO_SPEC_SHARDS", s.no_spec_shards},
      {"MVUS_SQ_DEVICE_SUM", s.sq_device_sum}, {"MVUS_LSMR_HOST", s.lsmr_host}, {"MVUS_LSMR_BOUNDED_HOST", s.lsmr_bounded_host},
      {"MVUS_LSMR_ONE_PASS", s.lsmr_one_pass}, {"MVUS_LSMR_TRACE", s.lsmr_trace}, {"MVUS_GEMM_SLABS", s.gemm_slabs}, {"MVUS_RCS", s.rcs_gj},
      {"MVUS_RCS_TRSM", s.rcs_trsm_launch}, {"MVUS_RCS_SPIN_LIMIT", s.rcs_spin_limit}, {"MVUS_BCR_FUSED", s.bcr_fused},
      {"MVUS_PART_LEN", s.part_len}, {"MVUS_PART_BACK", s.part_back}, {"MVUS_DIRECT_RHS", s.direct_rhs},
      {"MVUS_SEP_SEQUENTIAL", s.sep_sequential}, {"MVUS_SEP_TWO_LEVEL", s.sep_two_level}, {"MVUS_ASM_ATOMIC", s.asm_atomic},
      {"MVUS_WIN", s.win}, {"MVUS_WIN_GROUPS", s.win_groups}, {"MVUS_NO_SPEC", s.no_spec}, {"MVUS_LM_MATERIALIZE_J", s.lm_materialize_j},
      {"MVUS_NE_FROM_J", s.ne_from_j}, {"MVUS_NO_OVERLAP", s.no_overlap}, {"MVUS_DEBUG", s.debug}};
  for (const auto& f : fields) if (std::strcmp(f.name, name) == 0) return f.value;
  return -2;
}
