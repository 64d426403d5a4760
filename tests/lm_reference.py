"""LAPACK reference for one damped Gauss-Newton step of the LM + Schur solver, from the normal-equation blocks the
library exports (mvus_ba_normal_equations): banded Cholesky of the spline block, dense Schur complement on the camera
block.  Test infrastructure (checks mvus_ba_lm_step, i.e. the whole GPU solve chain)."""
import numpy as np


def lapack_lm_step(prob, g, A, band, cross, lam):
    """p = -(H + lam * D)^-1 g with H = [[A, E], [E^T, C]] given as camera blocks A[C,B,B], block band[N,W,3,3] and
    cross[C,B,3N]; D = diag(H) (1 where 0)."""
    from scipy.linalg import solveh_banded
    C, B, N, W = prob.C, 3 + prob.P, band.shape[0], band.shape[1]
    cam_cols = np.array([[c, C + c, 2 * C + c] + list(range(3 * C + c * prob.P, 3 * C + (c + 1) * prob.P)) for c in range(C)])
    spl_cols = np.concatenate([[int(prob.spline_x_offsets[s_]) + d * int(n_) + j for j in range(int(n_)) for d in range(3)]
                               for s_, n_ in enumerate(prob.n_coef)])
    bw = 3 * W - 1
    ab = np.zeros((bw + 1, 3 * N))                                  # upper banded storage of the spline block
    for w in range(W):
        for a_ in range(3):
            for b_ in range(3):
                off = 3 * w + b_ - a_
                if off < 0:
                    continue
                rows = 3 * np.arange(N - w) + a_
                ab[bw - off, rows + off] = band[:N - w, w, a_, b_]
    dS = ab[bw].copy()
    ab[bw] += lam * np.where(dS > 0, dS, 1.0)
    Esp = cross.reshape(C * B, 3 * N)
    Z = solveh_banded(ab, np.column_stack([Esp.T, g[spl_cols]]))
    Acam = np.zeros((C * B, C * B))
    for c in range(C):
        Acam[c * B:(c + 1) * B, c * B:(c + 1) * B] = A[c]
    dA = np.diag(Acam).copy()
    Sred = Acam + lam * np.diag(np.where(dA > 0, dA, 1.0)) - Esp @ Z[:, :-1]
    pc = -np.linalg.solve(Sred, g[cam_cols.ravel()] - Esp @ Z[:, -1])
    ps = -(Z[:, -1] + Z[:, :-1] @ pc)
    p = np.zeros(prob.n_params)
    p[cam_cols.ravel()] = pc
    p[spl_cols] = ps
    return p


# The two conditions every GPU step is held to (schur_reference.eta: backward error on the Jacobi-scaled system):
#   eta <= ETA_FACTOR * max(eta of lapack_lm_step on the same blocks, ETA_FLOOR)   -- relative to the reference, never to the code under test;
#          the floor is the median eta of LAPACK on the host systems of test_schur_reference_host.py (a lucky 5e-18 does not set the bar),
#          the factor an allowance for explicit block inverses and log2 levels of cyclic reduction over a banded Cholesky
#   eta <= ETA_CAP   -- a condition, not a measurement: the weakest sixth-digit fault of test_schur_reference_host.py sits at 6e-10, the
#          reference below 1e-13; above the cap a test no longer separates the two.  No route is exempt from it.
ETA_FACTOR = 64.0
ETA_FLOOR = 1e-15
ETA_CAP = 1e-11

# The solve routes the step tests run (test_gpu_schur_backward_error.py, test_gpu_rcs.py): name -> the switches of ba_switches.h that select it
SOLVE_ROUTES = {
    'default': {},
    # the reduced camera system
    'rcs_gj': {'MVUS_RCS': 'gj'},
    'rcs_trsm_launch': {'MVUS_RCS_TRSM': 'launch'},
    # the separator system
    'sep_sequential': {'MVUS_SEP_SEQUENTIAL': '1'},
    # the band solver
    'part_back': {'MVUS_PART_BACK': '1'},
    'rhs_copy': {'MVUS_DIRECT_RHS': '0'},
    'no_overlap': {'MVUS_NO_OVERLAP': '1'},
    'part_len_16': {'MVUS_PART_LEN': '16'},
    'part_len_32': {'MVUS_PART_LEN': '32'},
    # the Schur product
    'slabs_1': {'MVUS_GEMM_SLABS': '1'},
    'slabs_3': {'MVUS_GEMM_SLABS': '3'},
    'slabs_8': {'MVUS_GEMM_SLABS': '8'},
    # interiors of two separators' length: the longest separator chain a spline can have, several reduction levels at a tiny size; with
    # 68 or more separators two of the levels are wide, and those run in one launch (k_sep_bcr_levels) or, MVUS_BCR_FUSED=0, in one each
    'part_len_6': {'MVUS_PART_LEN': '6'},
    'part_len_6_sequential': {'MVUS_PART_LEN': '6', 'MVUS_SEP_SEQUENTIAL': '1'},
    'part_len_6_bcr_per_level': {'MVUS_PART_LEN': '6', 'MVUS_BCR_FUSED': '0'},
    # back-correction and right-hand-side copy over more than 128 columns (several column blocks of k_part_back), on a scene that has a
    # separator only with interiors of 16
    'part_len_16_part_back': {'MVUS_PART_LEN': '16', 'MVUS_PART_BACK': '1'},
    'part_len_16_rhs_copy': {'MVUS_PART_LEN': '16', 'MVUS_DIRECT_RHS': '0'},
}
# route: (factor, reason), where a route is by its construction further from LAPACK than
# ETA_FACTOR: 4 x the measured ratio, the reason also in DESIGN.md section 4.10.  The cap holds for these too.
ROUTE_FACTOR = {
    # k_gj_step multiplies by the EXPLICIT inverse of every 32 x 32 pivot block (pivot_inverse_wave): a solve through a computed inverse
    # has a backward error proportional to the condition number (Higham, Accuracy and Stability of Numerical Algorithms, section 14.1),
    # where L D L^T with substitutions does not.  Measured: eta_cam = 0.3 ... 0.9e-18 x kappa(S M S) at every lambda (1e-12 at lambda = 1e-4,
    # kappa 1e6; 5e-17 at 0.7, kappa 1e2), the spline rows as on the default route; worst ratio to LAPACK 378 (scene B, lambda = 1e-4).
    'rcs_gj': (4 * 378.0, 'explicit inverses of the pivot blocks: eta grows with kappa'),
}


assert set(ROUTE_FACTOR) <= set(SOLVE_ROUTES)


def route_factor(route):
    """The factor of assertion 1 for a route of SOLVE_ROUTES (a name that is not one is an error, not the default)."""
    if route not in SOLVE_ROUTES:
        raise KeyError('no such solve route: %r' % (route,))
    return ROUTE_FACTOR.get(route, (ETA_FACTOR, ''))[0]


def eta_bound(eta_ref, factor=ETA_FACTOR):
    return min(factor * max(eta_ref, ETA_FLOOR), ETA_CAP)


def backward_error(prob, g, A, band, cross, lam, p, what='', factor=ETA_FACTOR):
    """(eta of p, eta of lapack_lm_step, the bound p is held to) on these blocks, printed; the caller asserts or collects."""
    import schur_reference as sr
    e = sr.eta(prob, g, A, band, cross, lam, p)
    e_ref = sr.eta(prob, g, A, band, cross, lam, lapack_lm_step(prob, g, A, band, cross, lam))
    bound = eta_bound(e_ref.eta, factor)
    print('%s lambda %g: eta = %.3g (cam %.3g, spline %.3g), eta_ref = %.3g, ratio %.3g, bound %.3g'
          % (what, lam, e.eta, e.cam, e.spline, e_ref.eta, e.eta / max(e_ref.eta, ETA_FLOOR), bound))
    return e, e_ref, bound


def assert_backward_error(prob, g, A, band, cross, lam, p, what='', factor=ETA_FACTOR):
    e, e_ref, bound = backward_error(prob, g, A, band, cross, lam, p, what, factor)
    assert np.isfinite(e.eta) and e.eta <= bound, (what, lam, e, e_ref, bound)
    return e, e_ref
