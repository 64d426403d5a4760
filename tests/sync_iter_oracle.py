"""numpy / scipy restatement of the iterative time-shift search (csrc/sync_iter.hip.h, synchronization.sync_iter_gpu), for the tests
and tools/time_sync_iter.py.  Independent of the kernels where it can be: the pencil's eigenvalues from scipy.linalg.eigvals (QZ) with
the reference's iscomplex / isfinite filter, the 8-point fit from epipolar_oracle (LAPACK SVD), the track of camera 2 from splev.  What
must agree exactly is restated exactly: the counter-based sampler and the order of the selection.

Conventions (the library's): camera 2's spline is fitted once, on its own unshifted timeline t2; ``shift`` is the current estimate of
beta, so camera 2's samples lie at t2 + shift on camera 1's timeline.  A model is (F, mshift) with mshift = beta_eig * d; it is scored
at tau = t1 - shift + mshift on camera 2's timeline, and the round returns -mshift of the winner (the reference's -result[-1])."""
import numpy as np
from scipy import interpolate, linalg

import epipolar_oracle as eo
from mvus_amd.tools import util

M64 = (1 << 64) - 1
EPS = float(np.finfo(np.float64).eps)


def sample9(seed, rnd, sign, h, n):
    """si_sample9: nine distinct indices below n."""
    ctr = (seed * 0x100000001b3 + rnd * 0x9e3779b1 + sign * 0x632be5ab + h * 1000003 + 0x2545f4914f6cdd1d) & M64
    idx = []
    while len(idx) < 9:
        ctr = eo._mix(ctr)
        c = ctr % n
        if c not in idx:
            idx.append(c)
    return idx


def prepare(fps1, fps2, detect1, detect2, frame1, frame2):
    """The preprocessing of synchronization.py:85-92 with camera 2 left on its own timeline."""
    alpha = fps1 / fps2
    d1 = np.vstack((detect1[0] / alpha, detect1[1:3])).astype(np.float64)
    d2 = np.asarray(detect2[:3], dtype=np.float64)
    tck1, _ = interpolate.splprep(d1[1:], u=d1[0], s=0, k=3)
    tck2, _ = interpolate.splprep(d2[1:], u=d2[0], s=0, k=3)
    return dict(alpha=alpha, beta_prior=frame1 / alpha - frame2, d1=d1, t2=d2[0].copy(), tck1=tck1, tck2=tck2,
                intervals=util.find_intervals(d2[0]), n=min(d1.shape[1], d2.shape[1]))


def samples(prep, shift, d, idx):
    """s1, s2, ds (2 x 9) of the nine samples idx of camera 2."""
    u = prep['t2'][np.asarray(idx)]
    s1 = np.asarray(interpolate.splev(u + shift, prep['tck1']))
    s2 = np.asarray(interpolate.splev(u, prep['tck2']))
    ds = np.asarray(interpolate.splev(u + d, prep['tck2'])) - s2
    return s1, s2, ds


def pencil(s1, s2, ds):
    one, zero = np.ones(9), np.zeros(9)
    A1 = np.array([s1[0] * s2[0], s1[0] * s2[1], s1[0], s1[1] * s2[0], s1[1] * s2[1], s1[1], s2[0], s2[1], one]).T
    A2 = np.array([s1[0] * ds[0], s1[0] * ds[1], zero, s1[1] * ds[0], s1[1] * ds[1], zero, ds[0], ds[1], zero]).T
    return A1, A2


def pencil_betas(A1, A2):
    """The finite real beta with det(A1 + beta A2) = 0, ascending: the reference's filter on -eigvals(A1, A2)."""
    if not (np.all(np.isfinite(A1)) and np.all(np.isfinite(A2))):
        return np.zeros(0)
    with np.errstate(all='ignore'):
        w = -linalg.eigvals(A1, A2)
    w[np.iscomplex(w)] = np.inf
    return np.sort(w.real[np.isfinite(w)])


def settled_hypothesis(A1, A2, rng, copies=4, rel=1e-13):
    """The same number of real eigenvalues for the pencil and for copies perturbed by rel."""
    n = len(pencil_betas(A1, A2))
    for _ in range(copies):
        P1 = A1 * (1.0 + rel * rng.uniform(-1, 1, A1.shape))
        P2 = A2 * (1.0 + rel * rng.uniform(-1, 1, A2.shape))
        if len(pencil_betas(P1, P2)) != n:
            return False
    return True


def kappa(A1, A2, betas):
    """Per beta: |x||y| (|A1|_F + |beta||A2|_F) / |y^H A2 x| from scipy's left and right eigenvectors."""
    with np.errstate(all='ignore'):
        w, vl, vr = linalg.eig(A1, A2, left=True, right=True)
    n1, n2 = np.linalg.norm(A1), np.linalg.norm(A2)
    out = []
    for b in betas:
        k = int(np.argmin(np.where(np.isfinite(w), np.abs(-w - b), np.inf)))
        x, y = vr[:, k], vl[:, k]
        out.append(np.linalg.norm(x) * np.linalg.norm(y) * (n1 + abs(b) * n2) / abs(np.vdot(y, A2 @ x)))
    return np.array(out)


def fit_F(s1, x2):
    """The normalised 8-point fit of the nine pairs, x2^T F s1 = 0: unit norm, F[2, 2] >= 0."""
    return eo.eight_point(s1, x2, eo.hartley_normalisation(s1), eo.hartley_normalisation(x2))


def hypothesis_models(prep, shift, d, idx):
    """[(beta, F)] of one hypothesis, beta ascending."""
    if len(set(prep['t2'][np.asarray(idx)].tolist())) < 9:
        return []
    s1, s2, ds = samples(prep, shift, d, idx)
    if not (np.all(np.isfinite(s1)) and np.all(np.isfinite(s2)) and np.all(np.isfinite(ds))):
        return []
    out = []
    for b in pencil_betas(*pencil(s1, s2, ds)):
        out.append((b, fit_F(s1, s2 + b * ds)))
    return out


def sampson(F, x1, x2):
    """epipolar.py:258-265 on 2 x N pixels."""
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    h1, h2 = np.vstack((x1, np.ones(x1.shape[1]))), np.vstack((x2, np.ones(x2.shape[1])))
    Fx1, Fx2 = F @ h1, F.T @ h2
    w = Fx1[0] ** 2 + Fx1[1] ** 2 + Fx2[0] ** 2 + Fx2[1] ** 2
    with np.errstate(all='ignore'):
        return np.sum(h2 * Fx1, axis=0) ** 2 / w


def score(prep, shift, F, mshift, threshold, detail=False):
    """(inliers, overlap) of one model."""
    d1 = prep['d1']
    tau = d1[0] - shift + mshift
    iv = prep['intervals']
    inside = np.zeros(tau.shape, dtype=bool)
    for k in range(iv.shape[1]):
        inside |= (tau >= iv[0, k]) & (tau < iv[1, k])
    if not inside.any():
        return (0, 0, tau, None) if detail else (0, 0)
    x2 = np.asarray(interpolate.splev(tau[inside], prep['tck2']))
    err = sampson(F, d1[1:3, inside], x2)
    with np.errstate(invalid='ignore'):
        inl = int(np.sum(err < threshold))
    return (inl, int(inside.sum()), tau, err) if detail else (inl, int(inside.sum()))


def settled_model(prep, shift, F, mshift, threshold, tol=1e-9):
    """No camera-1 timestamp within tol frames of an interval edge, no error within tol (relative) of the threshold."""
    _, ovl, tau, err = score(prep, shift, F, mshift, threshold, detail=True)
    edges = np.asarray(prep['intervals'], dtype=np.float64).reshape(-1)
    if edges.size and np.min(np.abs(tau[:, None] - edges[None, :])) <= tol:
        return False
    if err is not None and np.any(np.abs(err[np.isfinite(err)] - threshold) <= tol * threshold):
        return False
    return True


def round_(prep, shift, d, H, threshold, seed, rnd):
    """Both signs of d: [(beta_temp, ratio, inliers, overlap)] for +d and -d.  Strict >, in (hypothesis, slot) order, from 0."""
    out = []
    for sign in (0, 1):
        dd = -d if sign else d
        n = prep['n'] - 2 * abs(d)
        if n < 9:
            raise ValueError('fewer than nine samples')
        best = (0.0, 0.0, 0, 0)
        for h in range(H):
            for b, F in hypothesis_models(prep, shift, dd, sample9(seed, rnd, sign, h, n)):
                inl, ovl = score(prep, shift, F, b * dd, threshold)
                if ovl > 0 and inl / ovl > best[1]:
                    best = (-(b * dd), inl / ovl, inl, ovl)
        out.append(best)
    return out


def outer_loop(round_fn, beta_prior, alpha, step=10, p_min=0, p_max=6, verbose=False):
    """synchronization.py:95-130 around round_fn(shift, d, round_number) -> [(beta_temp, ratio, ...)] * 2."""
    skip, max_inlier, k = 0, 0, 0
    d, p, beta = 2 ** p_min, p_min, beta_prior
    rnd = 0
    while k < step:
        (beta1, inlier1, *_), (beta2, inlier2, *_) = round_fn(beta, d, rnd)
        rnd += 1
        beta_temp = beta1 if inlier1 >= inlier2 else beta2
        inlier = inlier1 if inlier1 >= inlier2 else inlier2
        if verbose:
            print('d:{}, beta:{:.3f}, maxInlier:{}, Inlier:{}'.format(d, (beta + beta_temp) * alpha, max_inlier, inlier))
        if skip > p_max:
            break
        elif inlier < max_inlier:
            p = p + 1 if p < p_max else 0
            d = 2 ** p
            skip += 1
        else:
            beta += beta_temp
            max_inlier = inlier
            skip = 0
            k += 1
    return beta * alpha, max_inlier


def sync_iter(fps1, fps2, detect1, detect2, frame1, frame2, maxIter=200, threshold=10, step=10, p_min=0, p_max=6, verbose=False, seed=0):
    prep = prepare(fps1, fps2, detect1, detect2, frame1, frame2)
    fn = lambda shift, d, rnd: round_(prep, shift, d, maxIter, threshold, seed, rnd)
    return outer_loop(fn, prep['beta_prior'], prep['alpha'], step, p_min, p_max, verbose)


# ---- the test scene ------------------------------------------------------------------------------------------------------------
def scene_pair(seed=32, moved=20.0):
    """Cameras 0 and 1 of synth.make_scene(2, 3000, seed): (fps1, fps2, detect1, detect2, frame1, frame2, true beta of camera 1) with
    camera 1's corresponding frame moved by ``moved`` frames off the truth."""
    from mvus_amd import synth
    sc = synth.make_scene(2, 3000, seed=seed)
    tr = sc.truth
    cf = -np.asarray(tr['beta'], dtype=np.float64) / np.asarray(tr['alpha'], dtype=np.float64)
    cf[1] += moved
    return (sc.cameras[0]['fps'], sc.cameras[1]['fps'], np.asarray(sc.detections[0], dtype=np.float64),
            np.asarray(sc.detections[1], dtype=np.float64), cf[0], cf[1], float(tr['beta'][1]), sc)
