"""tests/schur_reference.py against dense long-double algebra, on systems from the host build's dense Jacobian (no GPU).

The GPU tests of the LM + Schur step (test_gpu_schur_backward_error.py) rest on this file: the blockwise residual is the dense one,
LAPACK and the refined solve have the backward errors the GPU bounds are relative to, and steps that are wrong in the sixth digit --
which the older criterion |p - p_ref|_max <= 1e-7 |p_ref|_max lets through -- are caught."""
import functools

import numpy as np
import pytest

import schur_reference as sr
from lm_reference import lapack_lm_step
from mvus_amd import _lib
from mvus_amd import problem as mp

LD = np.longdouble
SCENES = {
    'A': dict(num_cam=3, total_obs=1200, seed=103, num_knots=40),
    'B': dict(num_cam=5, total_obs=1400, seed=105, num_knots=64, opt_calib=True),
    'C': dict(num_cam=17, total_obs=1420, seed=117, num_knots=24),
}
LAMS = (1e-4, 1e-3, 0.7)


@functools.lru_cache(maxsize=None)
def system(name):
    """(prob, (g, A, band, cross), H) of a scene: H = J^T J and g = J^T f of the host build's dense analytic Jacobian, cut into blocks."""
    from hostcheck_util import HostHandle
    from mvus_amd import synth
    sc = synth.make_scene(rolling_shutter=True, **SCENES[name])
    prob, x0 = mp.problem_from_scene(sc)
    f, J = HostHandle(prob).dense_jacobian(x0, _lib.JAC_ANALYTIC)
    H, grad = J.T @ J, J.T @ f
    blocks = sr.blocks_from_dense(prob, H, grad)
    assert np.array_equal(sr.dense(prob, *blocks), H)              # cutting and rebuilding loses nothing
    return prob, blocks, H


@functools.lru_cache(maxsize=None)
def lapack(name, lam):
    prob, blocks, _ = system(name)
    return lapack_lm_step(prob, *blocks, lam)


def test_scene_sizes():
    assert system('B')[0].n_params == 291 and system('B')[1][1].shape[1:] == (18, 18)
    assert system('A')[0].P == 6 and system('C')[0].C * (3 + system('C')[0].P) == 153


@pytest.mark.parametrize('lam', LAMS)
@pytest.mark.parametrize('name', sorted(SCENES))
def test_blockwise_residual_is_the_dense_one(name, lam):
    """(a) r = M p + g block by block against the dense product, to 4 long-double ulps of |M||p| + |g|, for the LAPACK step (where r
    cancels to rounding level) and for a random p (where it does not).  Two long-double sums of some hundred terms in different orders
    differ by about that much themselves (1.01 of the bound was seen), so the dense side is summed without error: every row of the dense
    M, the damping included, in rational arithmetic.  The 4 ulps are then all the blockwise function's."""
    from fractions import Fraction
    prob, blocks, H = system(name)
    n = prob.n_params
    d = np.diag(H)
    D = np.where(d > 0, d, 1.0)
    fl, g = Fraction(float(lam)), blocks[0]
    rng = np.random.default_rng(7)
    for p in (lapack(name, lam), rng.normal(size=n) * np.abs(lapack(name, lam)).max()):
        r = sr.residual(prob, *blocks, lam, p)
        assert r.dtype == LD and r.shape == (n,)
        pf = [Fraction(float(v)) for v in p]
        worst = 0.0
        for i in range(n):
            cols = np.nonzero(H[i])[0]
            exact = Fraction(float(g[i])) + fl * Fraction(float(D[i])) * pf[i] + sum(Fraction(float(H[i, j])) * pf[j] for j in cols)
            size = abs(Fraction(float(g[i]))) + fl * Fraction(float(D[i])) * abs(pf[i]) + sum(abs(Fraction(float(H[i, j])) * pf[j]) for j in cols)
            hi = float(r[i])
            got = Fraction(hi) + Fraction(float(r[i] - LD(hi)))                  # (a long double is the exact sum of two doubles)
            worst = max(worst, float(abs(got - exact) / (4 * Fraction(float(np.finfo(LD).eps)) * size)))
        print('%s lambda %g: |r_block - r_dense| / (4 ulp (|M||p| + |g|)) = %.3g' % (name, lam, worst))
        assert worst <= 1.0


@pytest.mark.parametrize('lam', LAMS)
@pytest.mark.parametrize('name', sorted(SCENES))
def test_reference_solvers_backward_error(name, lam):
    """(b) eta of lapack_lm_step and of np.linalg.solve <= 1e-13 (a condition on the reference alone: about 10 x what was measured);
    (c) eta of the refined solve <= 1e-18; (e) forward_scaled(p, p*) <= 2 kappa eta, the standard perturbation bound, for both."""
    prob, blocks, H = system(name)
    p_star = sr.refined(prob, *blocks, lam)
    e_star = sr.eta(prob, *blocks, lam, p_star)
    k = sr.kappa(prob, *blocks, lam)
    print('%s lambda %g: kappa = %.3g, eta(refined) = %.3g' % (name, lam, k, e_star.eta))
    assert p_star.dtype == LD and e_star.eta <= 1e-18
    for what, p in (('lapack_lm_step', lapack(name, lam)), ('np.linalg.solve', -np.linalg.solve(sr.damped(H, lam), blocks[0]))):
        e = sr.eta(prob, *blocks, lam, p)
        fwd = sr.forward_scaled(prob, *blocks, lam, p, p_star)
        print('  %-15s eta = %.3g (cam %.3g, spline %.3g), forward = %.3g, 2 kappa eta = %.3g' % (what, e.eta, e.cam, e.spline, fwd, 2 * k * e.eta))
        assert e.eta == max(e.cam, e.spline) and e.eta <= 1e-13
        assert fwd <= 2 * k * e.eta


def _mutant_spline(prob, blocks, lam, p):
    """One control point (three components) of the step times (1 + 1e-6)."""
    _, spl = sr.internal_index(prob)
    k = blocks[2].shape[0] // 2
    q = p.copy()
    q[spl[3 * k:3 * k + 3]] *= 1 + 1e-6
    return q


def _mutant_camera(prob, blocks, lam, p):
    """Camera 0's first three unknowns (two angles and the rolling-shutter fraction) times (1 + 1e-6)."""
    cam, _ = sr.internal_index(prob)
    q = p.copy()
    q[cam[0][:3]] *= 1 + 1e-6
    return q


def _mutant_band(prob, blocks, lam, p):
    """A step computed with one outermost band block dropped: band[k, W - 1] = 0."""
    g, A, band, cross = blocks
    k, W = band.shape[0] // 2, band.shape[1]
    assert np.abs(band[k, W - 1]).max() > 0
    cut = band.copy()
    cut[k, W - 1] = 0
    return lapack_lm_step(prob, g, A, cut, cross, lam)


# (mutant, scene, lambda) where the mutant moves the max-norm criterion of the older tests by MORE than 1e-7, i.e. where those tests
# would notice too: only the eta half is asserted there.  Everywhere else both halves are: caught by eta, invisible to the max-norm.
# Measured: the camera mutant on A (1e-6: the largest entry of p is one of camera 0's angles) and on C (3e-7), at every lambda; the dropped
# band block on every scene and lambda (8e-7 ... 4e-3: a whole block is no sixth-digit fault, it is here for the eta half).  The spline
# mutant everywhere, and the camera mutant on B, pass the max-norm criterion: 1e-10 ... 5e-8.
MAXNORM_SEES_IT = {('camera', s, lam) for s in 'AC' for lam in LAMS} | {('band', s, lam) for s in 'ABC' for lam in LAMS}


@pytest.mark.parametrize('lam', LAMS)
@pytest.mark.parametrize('name', sorted(SCENES))
@pytest.mark.parametrize('mutant', [_mutant_spline, _mutant_camera, _mutant_band], ids=['spline', 'camera', 'band'])
def test_sixth_digit_faults_fail_eta_and_pass_the_max_norm(mutant, name, lam):
    """(d) the blind spot, documented: each mutant has eta >= 1e-10 -- four orders above the reference -- while the criterion
    |q - p|_max / |p|_max of the older tests moves by less than its 1e-7."""
    prob, blocks, _ = system(name)
    p = lapack(name, lam)
    q = mutant(prob, blocks, lam, p)
    e = sr.eta(prob, *blocks, lam, q)
    moved = float(np.abs(q - p).max() / np.abs(p).max())
    print('%s %s lambda %g: eta = %.3g (cam %.3g, spline %.3g), max-norm moved by %.3g' % (mutant.__name__, name, lam, e.eta, e.cam, e.spline, moved))
    assert e.eta >= 1e-10
    if (mutant.__name__[8:], name, lam) in MAXNORM_SEES_IT:
        assert moved >= 1e-7, 'the exemption is out of date'
    else:
        assert moved < 1e-7
