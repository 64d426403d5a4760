// TEST-ONLY host build of the position priors' row routines (mvus_amd/csrc/ba_prior_math.h): what k_prior_setup runs per lane at set
// time and what k_prior_cost / k_prior_ne evaluate per row, in sequence here so that tests/test_position_priors_host.py can pin the
// arithmetic without a GPU.
#include "../mvus_amd/csrc/ba_prior_math.h"

using namespace mvus;

extern "C" {

// k_prior_setup: interval[2 * S] (starts then ends), knot_off / ctrl_off [S + 1], the concatenated knots; ctrl[K], h[4 * K] out
void priorcheck_setup(int S, const double* interval, const int32_t* knot_off, const int32_t* ctrl_off, const double* knots, long long K,
                      const double* t, int32_t* ctrl, double* h) {
  SplineView sp{};
  sp.S = S; sp.istart = interval; sp.iend = interval + S; sp.knots = knots; sp.knot_off = knot_off; sp.ctrl_off = ctrl_off;
  for (long long k = 0; k < K; ++k) ctrl[k] = prior_setup_row(sp, t[k], h + 4 * k);
}

// S(t) - p of one prior: coordinate d of control point a at x[x0[a] + d * stride[a]]
void priorcheck_diff(const double* x, const int32_t* x0, const int32_t* stride, const double* h, const double* p, double* diff) {
  prior_diff(x, x0, stride, h, p, diff);
}

}  // extern "C"
