"""scipy as the reference of the robust losses (mvus_ba_set_loss), through its PUBLIC API only.

``least_squares(fun, x, jac, loss=L, f_scale=s, max_nfev=1)`` returns at x untouched: ``res.cost`` is the robust cost
0.5 s^2 sum rho((f_i / s)^2), ``res.grad`` = J^T (rho' f) and ``res.jac`` = diag(s_i) J with s_i = sqrt(max(rho' + 2 rho'' z, EPS))
(scipy/optimize/_lsq/common.py: scale_for_robust_loss_function).  One trap: scipy scales a dense Jacobian IN PLACE, so ``jac`` hands
out a fresh array on every call (returning the same array corrupts every later call without a word).

``closed_form`` is the table of the losses written out, used to pin the wrapper (tests/test_robust_loss_host.py) and for rho', which
the public API does not return by itself.  Test infrastructure."""
import numpy as np

LOSSES = ('linear', 'soft_l1', 'huber', 'cauchy', 'arctan')
ROBUST = LOSSES[1:]
EPS = np.finfo(float).eps


def scipy_at(f, J, loss, f_scale):
    """(cost, grad, scaled J) of scipy's least_squares for residuals f[m] and the dense Jacobian J[m, n] (None: cost only)."""
    from scipy.optimize import least_squares
    f = np.array(f, dtype=np.float64)
    if J is None:
        J = np.zeros((f.size, 1))
    J = np.asarray(J, dtype=np.float64)
    res = least_squares(lambda x: f.copy(), np.zeros(J.shape[1]), jac=lambda x: np.array(J, copy=True), loss=loss, f_scale=f_scale,
                        max_nfev=1, method='trf')
    assert np.array_equal(res.x, np.zeros(J.shape[1])) and np.array_equal(res.fun, f)      # at x untouched, res.fun raw
    return float(res.cost), np.array(res.grad), np.array(res.jac)


def scipy_cost(f, loss, f_scale):
    return scipy_at(f, None, loss, f_scale)[0]


def closed_form(f, loss, f_scale):
    """rho, rho', rho'' at z = (f / f_scale)^2, row by row."""
    z = (np.asarray(f, dtype=np.float64) / f_scale) ** 2
    if loss == 'linear':
        return z, np.ones_like(z), np.zeros_like(z)
    if loss == 'soft_l1':
        t = 1 + z
        return 2 * (np.sqrt(t) - 1), t ** -0.5, -0.5 * t ** -1.5
    if loss == 'huber':
        out = z <= 1
        zs = np.where(out, 1.0, z)
        return np.where(out, z, 2 * np.sqrt(zs) - 1), np.where(out, 1.0, zs ** -0.5), np.where(out, 0.0, -0.5 * zs ** -1.5)
    if loss == 'cauchy':
        return np.log1p(z), 1 / (1 + z), -1 / (1 + z) ** 2
    if loss == 'arctan':
        return np.arctan(z), 1 / (1 + z ** 2), -2 * z / (1 + z ** 2) ** 2
    raise ValueError(loss)


def weights(f, loss, f_scale):
    """rho'(z_i): the weight of every row in the gradient."""
    return closed_form(f, loss, f_scale)[1]


def closed_cost(f, loss, f_scale):
    return 0.5 * f_scale ** 2 * float(np.sum(closed_form(f, loss, f_scale)[0]))


def closed_scale(f, loss, f_scale):
    """(s_i, rho'_i): the row scale of the Jacobian and the weight."""
    z = (np.asarray(f, dtype=np.float64) / f_scale) ** 2
    _, d1, d2 = closed_form(f, loss, f_scale)
    return np.sqrt(np.maximum(d1 + 2 * d2 * z, EPS)), d1
