// The partitioned band solver of the spline fit: one lane per interior, a block-tridiagonal separator system between them.
#pragma once
#include "ba_math.h"      // hip_runtime.h under hipcc
#include "spline_band_parts.h"
#include "spline_band_solve.hip.h"      // PivotStats
#include "spline_dd.h"

namespace mvus {

// ---- the same systems, partitioned --------------------------------------------------------------------------------------
// k_band_solve is one dependent chain of n rows (0.4 us a row in fp64, 4.8 us in double-double: 31 ms for the 6 500 coefficients
// of a 3.3 M-sample trajectory, and ~50 such solves per fit).  k_band_solve_parts cuts the rows into P interiors separated by
// P - 1 separators of HB rows (interiors do not couple: half-bandwidth <= HB), one LANE per interior:
//   phase 1  every lane factors its interior A_p = L L^T and forward-solves the coupling columns to the separator on its left
//            (Y_L, dense), to the one on its right (Y_R, last HB rows only) and the three right-hand sides (y); what the
//            interior contributes to the separator system (Y^T Y, Y^T y) goes to a record per interior
//   phase 2  one lane: block-tridiagonal Cholesky of the separator system (HB x HB blocks), both substitutions
//   phase 3  every lane: L^T x = y - Y_L x_left - Y_R x_right
// One workgroup (P <= 256 lanes), __syncthreads between the phases.  The elimination ORDER differs from k_band_solve's, so
// the factor's diagonal is not FITPACK's a(i,1): out[0] is not written; the caller runs k_band_solve once per fit where
// fppara needs that sum (the initial p).  out[2], out[3] = smallest / largest pivot of all the factors (same use as before).
#if defined(__HIPCC__)
template <int HB> struct BandRec {                  // per interior (T units)
  static constexpr int GLL = 0, GRR = HB * HB, C = 2 * HB * HB, YR = 3 * HB * HB, GL = 4 * HB * HB, GR = 4 * HB * HB + 3 * HB, SIZE = 4 * HB * HB + 6 * HB;
};
template <int HB> struct BandSep {                  // per separator (T units): its Cholesky block, the coupling W to the next one, z, x
  static constexpr int LT = 0, W = HB * HB, Z = 2 * HB * HB, X = 2 * HB * HB + 3 * HB, SIZE = 2 * HB * HB + 6 * HB;
};
constexpr int kBandPartsWork = kBandPartsMax * (BandRec<4>::SIZE + BandSep<4>::SIZE);        // T units of `work`

template <int HB, class T>
__global__ __launch_bounds__(kBandPartsMax) void k_band_solve_parts(int n, BandParts bp, const T* __restrict__ M, const T* __restrict__ rhs, T* __restrict__ Mt,
                                                                    T* __restrict__ rt, T* __restrict__ YL, T* __restrict__ work, double* __restrict__ c,
                                                                    double* __restrict__ out, int* __restrict__ fail) {
  // M, rhs: the system as the other kernels hold it (separator rows are read from there); Mt, rt: the interiors' rows transposed
  // (written by k_fit_band / k_fit_combine) -- overwritten in place by L and y, then by nothing: x goes straight to c
  constexpr int NW = HB + 1;
  using R = BandRec<HB>;
  using S = BandSep<HB>;
  constexpr int NC = HB + 3;                          // forward columns of an interior: HB couplings to the left, 3 right-hand sides
  const int p = threadIdx.x, P = bp.P;
  T* rec = work;
  T* sep = work + (long long)kBandPartsMax * R::SIZE;
  __shared__ double s_min[kBandPartsMax], s_max[kBandPartsMax];
  __shared__ int s_bad[kBandPartsMax];
  PivotStats<T> ps;
  const int r0 = p < P ? bp.first(p) : 0, lp = p < P ? bp.length(p) : 0;
  // ---- phase 1 ----
  if (p < P) {
    T Lp[HB + 1][HB + 1];                             // Lp[u][w] = L(i-u, i-u-w)
    T ip[HB + 1];                                     // ip[u] = 1 / L(i-u, i-u)
    T Yp[HB + 1][NC];                                 // Yp[u][col] = Y(i-u, col)
    T gll[HB][HB], gl[HB][3];
#pragma unroll
    for (int u = 0; u <= HB; ++u) {
      ip[u] = T(1.0);
#pragma unroll
      for (int w = 0; w <= HB; ++w) Lp[u][w] = (w == 0) ? T(1.0) : T(0.0);
#pragma unroll
      for (int col = 0; col < NC; ++col) Yp[u][col] = T(0.0);
    }
#pragma unroll
    for (int a = 0; a < HB; ++a) {
#pragma unroll
      for (int b = 0; b < HB; ++b) gll[a][b] = T(0.0);
#pragma unroll
      for (int d = 0; d < 3; ++d) gl[a][d] = T(0.0);
    }
    // rows are fetched RB at a time (all loads of a batch in flight together): with one row ahead every row waited a full memory
    // round trip (~0.7 us against ~0.15 us of fp64 arithmetic)
    constexpr int RB = sizeof(T) == sizeof(double) ? 8 : 2;
    for (int i0 = 0; i0 < lp; i0 += RB) {
     T cm[RB][HB + 1], cb[RB][3];
#pragma unroll
     for (int r = 0; r < RB; ++r) {
       const int ii = i0 + r < lp ? i0 + r : lp - 1;
#pragma unroll
       for (int w = 0; w <= HB; ++w) cm[r][w] = Mt[bp.at(p, ii, w, NW)];
#pragma unroll
       for (int d = 0; d < 3; ++d) cb[r][d] = rt[bp.at(p, ii, d, 3)];
     }
#pragma unroll
     for (int r = 0; r < RB; ++r) {
      const int i = i0 + r;
      if (i >= lp) break;
      T row[HB + 1], b[NC];
#pragma unroll
      for (int w = 0; w <= HB; ++w) row[w] = cm[r][w];
#pragma unroll
      for (int col = 0; col < HB; ++col) b[col] = T(0.0);
#pragma unroll
      for (int d = 0; d < 3; ++d) b[HB + d] = cb[r][d];
      if (i < HB) {                                   // M(j, j-w) with i - w < 0 couples to the separator on the left: column i + HB - w of it
#pragma unroll
        for (int w = 1; w <= HB; ++w) {
          if (w > i) {
#pragma unroll
            for (int col = 0; col < HB; ++col) if (col == i + HB - w) b[col] = row[w];
            row[w] = T(0.0);
          }
        }
      }
#pragma unroll
      for (int w = HB; w >= 1; --w) {                 // L(i, i-w)
        T v = row[w];
#pragma unroll
        for (int u2 = w + 1; u2 <= HB; ++u2) v -= row[u2] * Lp[w][u2 - w];
        row[w] = v * ip[w];
      }
      const T full = row[0];
      T dg = row[0];
#pragma unroll
      for (int u2 = 1; u2 <= HB; ++u2) dg -= row[u2] * row[u2];
      row[0] = ps.pivot(dg, full);
      const T inv = num_recip(row[0]);
      T y[NC];
#pragma unroll
      for (int col = 0; col < NC; ++col) {
        T v = b[col];
#pragma unroll
        for (int u2 = 1; u2 <= HB; ++u2) v -= row[u2] * Yp[u2][col];
        y[col] = v * inv;
      }
#pragma unroll
      for (int a = 0; a < HB; ++a) {
#pragma unroll
        for (int b2 = 0; b2 <= a; ++b2) gll[a][b2] += y[a] * y[b2];
#pragma unroll
        for (int d = 0; d < 3; ++d) gl[a][d] += y[a] * y[HB + d];
      }
#pragma unroll
      for (int w = 0; w <= HB; ++w) Mt[bp.at(p, i, w, NW)] = row[w];
#pragma unroll
      for (int col = 0; col < HB; ++col) YL[bp.at(p, i, col, HB)] = y[col];
#pragma unroll
      for (int d = 0; d < 3; ++d) rt[bp.at(p, i, d, 3)] = y[HB + d];
#pragma unroll
      for (int u2 = HB; u2 >= 2; --u2) {
        ip[u2] = ip[u2 - 1];
#pragma unroll
        for (int w = 0; w <= HB; ++w) Lp[u2][w] = Lp[u2 - 1][w];
#pragma unroll
        for (int col = 0; col < NC; ++col) Yp[u2][col] = Yp[u2 - 1][col];
      }
      ip[1] = inv;
#pragma unroll
      for (int w = 0; w <= HB; ++w) Lp[1][w] = row[w];
#pragma unroll
      for (int col = 0; col < NC; ++col) Yp[1][col] = y[col];
     }
    }
    T* rc = rec + (long long)p * R::SIZE;
#pragma unroll
    for (int a = 0; a < HB; ++a) {
#pragma unroll
      for (int b2 = 0; b2 < HB; ++b2) rc[R::GLL + a * HB + b2] = b2 <= a ? gll[a][b2] : gll[b2][a];
#pragma unroll
      for (int d = 0; d < 3; ++d) rc[R::GL + a * 3 + d] = gl[a][d];
    }
    if (p + 1 < P) {
      // separator row r0 + lp + cq couples to the interior row lp - HB + r (window index u = HB - r) through M(., w = HB - r + cq):
      // Y_R(r, cq), lower triangular in (r, cq)
      const long long s0 = (long long)r0 + lp;
      T yr[HB][HB];
#pragma unroll
      for (int r = 0; r < HB; ++r) {
#pragma unroll
        for (int cq = 0; cq < HB; ++cq) {
          if (cq <= r) {
            T v = M[5 * (s0 + cq) + (HB - r + cq)];
#pragma unroll
            for (int r2 = 0; r2 < HB; ++r2) if (r2 >= cq && r2 < r) v -= Lp[HB - r][r - r2] * yr[r2][cq];
            yr[r][cq] = v * ip[HB - r];
          } else {
            yr[r][cq] = T(0.0);
          }
        }
      }
#pragma unroll
      for (int a = 0; a < HB; ++a) {
#pragma unroll
        for (int b2 = 0; b2 < HB; ++b2) {
          T grr = T(0.0), cc = T(0.0);
#pragma unroll
          for (int r = 0; r < HB; ++r) { grr += yr[r][a] * yr[r][b2]; cc += Yp[HB - r][a] * yr[r][b2]; }
          rc[R::GRR + a * HB + b2] = grr;
          rc[R::C + a * HB + b2] = cc;                // C(a, b2) = sum_i Y_L(i, a) Y_R(i, b2)
          rc[R::YR + a * HB + b2] = yr[a][b2];
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          T g = T(0.0);
#pragma unroll
          for (int r = 0; r < HB; ++r) g += yr[r][a] * Yp[HB - r][HB + d];
          rc[R::GR + a * 3 + d] = g;
        }
      }
    }
  }
  __syncthreads();
  __threadfence_block();
  // ---- phase 2: the separator system: lanes 0..2 of the first wavefront, one right-hand side each (the matrix part is the same
  // arithmetic in all three; lane 0 stores it).  The inputs of separator q + 1 are fetched while separator q is processed: a step
  // was 2.6 us (fp64), one memory round trip of it waiting for ~60 loads.
  if (p < 3) {
    const int dcol = p;
    struct SepIn { T grr[HB][HB], gll[HB][HB], cm[HB][HB], m[HB][HB], gr[HB], gl[HB], rh[HB]; };
    auto load_sep = [&](int q, SepIn& in) {
      const long long s0 = (long long)bp.first(q) + bp.length(q);
      const T* ra = rec + (long long)q * R::SIZE;
      const T* rb = rec + (long long)(q + 1) * R::SIZE;
#pragma unroll
      for (int a = 0; a < HB; ++a) {
#pragma unroll
        for (int b2 = 0; b2 < HB; ++b2) {
          in.grr[a][b2] = b2 <= a ? ra[R::GRR + a * HB + b2] : T(0.0);
          in.gll[a][b2] = b2 <= a ? rb[R::GLL + a * HB + b2] : T(0.0);
          in.cm[a][b2] = rb[R::C + a * HB + b2];
          in.m[a][b2] = b2 <= a ? M[5 * (s0 + a) + (a - b2)] : T(0.0);
        }
        in.gr[a] = ra[R::GR + a * 3 + dcol];
        in.gl[a] = rb[R::GL + a * 3 + dcol];
        in.rh[a] = rhs[(long long)dcol * n + s0 + a];
      }
    };
    T W[HB][HB], z[HB];
    PivotStats<T> ps2;                                // the separator pivots (lane 0 adds them to its statistics)
    // (fp64 only: in double-double the second set of blocks does not fit the register file -- 312 B of scratch per lane -- and the
    // arithmetic of a step, ~12 us, hides nothing worth hiding)
    constexpr bool kAhead = sizeof(T) == sizeof(double);
    SepIn nxt_in;
    if (kAhead && P > 1) load_sep(0, nxt_in);
    for (int q = 0; q + 1 < P; ++q) {
      SepIn in;
      if (kAhead) { in = nxt_in; if (q + 2 < P) load_sep(q + 1, nxt_in); }
      else load_sep(q, in);
      T D[HB][HB], full[HB], r[HB];
#pragma unroll
      for (int a = 0; a < HB; ++a) {
#pragma unroll
        for (int b2 = 0; b2 <= a; ++b2) {
          T v = in.m[a][b2] - in.grr[a][b2] - in.gll[a][b2];
          if (b2 == a) full[a] = in.m[a][a];
          if (q > 0) {
#pragma unroll
            for (int k = 0; k < HB; ++k) v -= W[a][k] * W[b2][k];
          }
          D[a][b2] = v;
        }
        T v = in.rh[a] - in.gr[a] - in.gl[a];
        if (q > 0) {
#pragma unroll
          for (int k = 0; k < HB; ++k) v -= W[a][k] * z[k];
        }
        r[a] = v;
      }
      T Lt[HB][HB], il[HB];
#pragma unroll
      for (int a = 0; a < HB; ++a) {
#pragma unroll
        for (int b2 = 0; b2 < a; ++b2) {
          T v = D[a][b2];
#pragma unroll
          for (int k = 0; k < HB; ++k) if (k < b2) v -= Lt[a][k] * Lt[b2][k];
          Lt[a][b2] = v * il[b2];
        }
        T dg = D[a][a];
#pragma unroll
        for (int k = 0; k < HB; ++k) if (k < a) dg -= Lt[a][k] * Lt[a][k];
        Lt[a][a] = ps2.pivot(dg, full[a]);
        il[a] = num_recip(Lt[a][a]);
        T v = r[a];
#pragma unroll
        for (int k = 0; k < HB; ++k) if (k < a) v -= Lt[a][k] * z[k];
        z[a] = v * il[a];
      }
      T* sq = sep + (long long)q * S::SIZE;
#pragma unroll
      for (int a = 0; a < HB; ++a) {
        if (dcol == 0) {
#pragma unroll
          for (int b2 = 0; b2 < HB; ++b2) sq[S::LT + a * HB + b2] = b2 < a ? Lt[a][b2] : (b2 == a ? il[a] : T(0.0));    // the diagonal holds 1 / L
        }
        sq[S::Z + a * 3 + dcol] = z[a];
      }
      if (q + 2 < P) {                                // W = O Lt^-T, O(cq, cc) = -C_{q+1}(cc, cq): rows = the next separator
#pragma unroll
        for (int a = 0; a < HB; ++a) {
#pragma unroll
          for (int k = 0; k < HB; ++k) {
            T v = -in.cm[k][a];
#pragma unroll
            for (int m2 = 0; m2 < HB; ++m2) if (m2 < k) v -= W[a][m2] * Lt[k][m2];
            W[a][k] = v * il[k];
          }
        }
        if (dcol == 0) {
#pragma unroll
          for (int a = 0; a < HB; ++a) {
#pragma unroll
            for (int k = 0; k < HB; ++k) sq[S::W + a * HB + k] = W[a][k];
          }
        }
      }
    }
    if (dcol == 0) { ps.dsum += ps2.dsum; ps.dmin = fmin(ps.dmin, ps2.dmin); ps.dmax = fmax(ps.dmax, ps2.dmax); ps.bad |= ps2.bad; }
    // lanes 1, 2 read what lane 0 stored (Lt, W): same wavefront, program order + the memory fence below
    __threadfence_block();
    T x[HB];
    struct SepBack { T lt[HB][HB], w[HB][HB], z[HB]; };
    auto load_back = [&](int q, SepBack& in) {
      const T* sq = sep + (long long)q * S::SIZE;
#pragma unroll
      for (int a = 0; a < HB; ++a) {
#pragma unroll
        for (int k = 0; k < HB; ++k) { in.lt[a][k] = sq[S::LT + a * HB + k]; in.w[a][k] = q + 2 < P ? sq[S::W + a * HB + k] : T(0.0); }
        in.z[a] = sq[S::Z + a * 3 + dcol];
      }
    };
    SepBack nxt_b;
    if (kAhead && P > 1) load_back(P - 2, nxt_b);
    for (int q = P - 2; q >= 0; --q) {                // x_q = Lt^-T (z_q - W_q^T x_{q+1}); the blocks of q - 1 are fetched meanwhile
      T* sq = sep + (long long)q * S::SIZE;
      SepBack in;
      if (kAhead) { in = nxt_b; if (q > 0) load_back(q - 1, nxt_b); }
      else load_back(q, in);
      T v[HB];
#pragma unroll
      for (int a = 0; a < HB; ++a) {
        T t = in.z[a];
        if (q + 2 < P) {
#pragma unroll
          for (int k = 0; k < HB; ++k) t -= in.w[k][a] * x[k];
        }
        v[a] = t;
      }
#pragma unroll
      for (int a = HB - 1; a >= 0; --a) {
        T t = v[a];
#pragma unroll
        for (int k = 0; k < HB; ++k) if (k > a) t -= in.lt[k][a] * x[k];
        x[a] = t * in.lt[a][a];
      }
      const long long s0 = (long long)bp.first(q) + bp.length(q);
#pragma unroll
      for (int a = 0; a < HB; ++a) { sq[S::X + a * 3 + dcol] = x[a]; c[(long long)dcol * n + s0 + a] = to_double(x[a]); }
    }
  }
  __syncthreads();
  __threadfence_block();
  // ---- phase 3 ----
  if (p < P) {
    T xl[HB][3], xr[HB][3], yr[HB][HB];
#pragma unroll
    for (int a = 0; a < HB; ++a) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        xl[a][d] = p > 0 ? sep[(long long)(p - 1) * S::SIZE + S::X + a * 3 + d] : T(0.0);
        xr[a][d] = p + 1 < P ? sep[(long long)p * S::SIZE + S::X + a * 3 + d] : T(0.0);
      }
#pragma unroll
      for (int b2 = 0; b2 < HB; ++b2) yr[a][b2] = p + 1 < P ? rec[(long long)p * R::SIZE + R::YR + a * HB + b2] : T(0.0);
    }
    T Ln[HB + 1][HB + 1], cn[HB + 1][3];              // Ln[u][w] = L(i+u, i+u-w), cn[u] = x(i+u)
#pragma unroll
    for (int u = 0; u <= HB; ++u) {
#pragma unroll
      for (int w = 0; w <= HB; ++w) Ln[u][w] = T(0.0);
#pragma unroll
      for (int d = 0; d < 3; ++d) cn[u][d] = T(0.0);
    }
    constexpr int RB = sizeof(T) == sizeof(double) ? 8 : 2;            // rows per batch of loads, as in phase 1
    for (int i1 = lp - 1; i1 >= 0; i1 -= RB) {
     T cm[RB][HB + 1], cyl[RB][HB], cy[RB][3];
#pragma unroll
     for (int r = 0; r < RB; ++r) {
       const int ii = i1 - r >= 0 ? i1 - r : 0;
#pragma unroll
       for (int w = 0; w <= HB; ++w) cm[r][w] = Mt[bp.at(p, ii, w, NW)];
#pragma unroll
       for (int col = 0; col < HB; ++col) cyl[r][col] = YL[bp.at(p, ii, col, HB)];
#pragma unroll
       for (int d = 0; d < 3; ++d) cy[r][d] = rt[bp.at(p, ii, d, 3)];
     }
#pragma unroll
     for (int r = 0; r < RB; ++r) {
      const int i = i1 - r;
      if (i < 0) break;
      const long long j = r0 + i;
      T row[HB + 1], yl[HB], v[3];
#pragma unroll
      for (int w = 0; w <= HB; ++w) row[w] = cm[r][w];
#pragma unroll
      for (int col = 0; col < HB; ++col) yl[col] = cyl[r][col];
#pragma unroll
      for (int d = 0; d < 3; ++d) v[d] = cy[r][d];
      const int rr = i - (lp - HB);                   // row of Y_R (>= 0 in the last HB rows of the interior)
      const T inv = num_recip(row[0]);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        T t = v[d];
#pragma unroll
        for (int col = 0; col < HB; ++col) t -= yl[col] * xl[col][d];
        if (rr >= 0) {
#pragma unroll
          for (int r = 0; r < HB; ++r) {
            if (r == rr) {
#pragma unroll
              for (int cq = 0; cq < HB; ++cq) t -= yr[r][cq] * xr[cq][d];
            }
          }
        }
#pragma unroll
        for (int u2 = 1; u2 <= HB; ++u2) t -= Ln[u2][u2] * cn[u2][d];
        t = t * inv;
        v[d] = t;
        c[(long long)d * n + j] = to_double(t);
      }
#pragma unroll
      for (int u2 = HB; u2 >= 2; --u2) {
#pragma unroll
        for (int w = 0; w <= HB; ++w) Ln[u2][w] = Ln[u2 - 1][w];
#pragma unroll
        for (int d = 0; d < 3; ++d) cn[u2][d] = cn[u2 - 1][d];
      }
#pragma unroll
      for (int w = 0; w <= HB; ++w) Ln[1][w] = row[w];
#pragma unroll
      for (int d = 0; d < 3; ++d) cn[1][d] = v[d];
     }
    }
  }
  s_min[p] = ps.dmin; s_max[p] = ps.dmax; s_bad[p] = ps.bad ? 1 : 0;
  __syncthreads();
  if (p == 0) {
    double mn = 1e300, mx = 0.0;
    int bad = 0;
    for (int k = 0; k < (int)blockDim.x; ++k) { mn = fmin(mn, s_min[k]); mx = fmax(mx, s_max[k]); bad |= s_bad[k]; }
    out[2] = mn; out[3] = mx;
    if (bad) fail[0] = 1;
  }
}
#endif

}  // namespace mvus
