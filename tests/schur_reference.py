"""Host reference for the damped step of the LM + Schur solver, on the blocks mvus_ba_normal_equations exports: g[n], A[C,B,B],
band[N,W,3,3] (band[i, w] = the 3x3 block of control points (i, i + w); the lower blocks are its mirror) and cross[C,B,3N].

    M = H + lam * D,   D = diag(H) with 1 where H has a zero,   S = diag(M)^(-1/2)

What is measured is the normwise backward error of a step p ON THE JACOBI-SCALED SYSTEM (Rigal and Gaches),

    eta = |S r|_inf / (|S M S|_inf |S^-1 p|_inf + |S g|_inf),   r = M p + g  in long double,

i.e. the size of the smallest relative change of (S M S, S g) that makes p an exact solution.  It does not depend on the units of the
unknowns (angles, pixels, metres share no scale), Cholesky-type eliminations of a definite matrix are stable in exactly this scaling,
and it needs no better solver as a reference, only a residual in extended precision.  Everything that touches a long chain works
block by block: no n x n array is formed except by dense(), refined() and kappa(), which are for n <= 1000.  numpy only.
Test infrastructure (checks mvus_ba_lm_step, i.e. the whole GPU solve chain)."""
from collections import namedtuple

import numpy as np

LD = np.longdouble
DENSE_MAX = 1000

Eta = namedtuple('Eta', 'eta cam spline')


def internal_index(prob):
    """x index of every unknown in the solver's internal order: camera blocks (alpha,beta,rs,params), then 3*ctrl+xyz."""
    C, P = prob.C, prob.P
    cam = [[c, C + c, 2 * C + c] + list(range(3 * C + c * P, 3 * C + (c + 1) * P)) for c in range(C)]
    spl = []
    for s, n in enumerate(prob.n_coef):
        for j in range(int(n)):
            spl += [int(prob.spline_x_offsets[s]) + d * int(n) + j for d in range(3)]
    return np.array(cam), np.array(spl)


class _System:
    """The damped system in long double, in the internal order (camera unknowns c * B + b, then 3 * ctrl + xyz)."""

    def __init__(self, prob, g, A, band, cross, lam):
        cam_idx, self.spl = internal_index(prob)
        self.cam = cam_idx.ravel()
        self.n = int(prob.n_params)
        self.C, self.B = A.shape[0], A.shape[1]
        self.N, self.W = band.shape[0], band.shape[1]
        self.CB, self.N3 = self.C * self.B, 3 * self.N
        assert cross.size == self.CB * self.N3 and self.cam.size == self.CB and self.spl.size == self.N3 and g.shape == (self.n,)
        self.A = np.asarray(A, dtype=np.float64).astype(LD)
        self.E = np.asarray(cross, dtype=np.float64).reshape(self.CB, self.N3).astype(LD)
        self.band = np.asarray(band, dtype=np.float64).astype(LD)
        for w in range(1, self.W):
            self.band[max(self.N - w, 0):, w] = 0              # (blocks past the end of the chain are not part of H)
        gl = np.asarray(g, dtype=np.float64).astype(LD)
        self.gc, self.gs = gl[self.cam], gl[self.spl]
        dc = np.einsum('cii->ci', self.A).reshape(-1)
        ds = np.einsum('nii->ni', self.band[:, 0]).reshape(-1)
        lam = LD(lam)
        self.damp_c = lam * np.where(dc > 0, dc, LD(1))         # lam * D
        self.damp_s = lam * np.where(ds > 0, ds, LD(1))
        self.sc = 1 / np.sqrt(dc + self.damp_c)                 # S
        self.ss = 1 / np.sqrt(ds + self.damp_s)

    def split(self, p):
        p = np.asarray(p).astype(LD)
        assert p.shape == (self.n,)
        return p[self.cam], p[self.spl]

    def join(self, vc, vs, dtype=LD):
        out = np.zeros(self.n, dtype=dtype)
        out[self.cam], out[self.spl] = vc, vs
        return out

    def matvec(self, pc, ps, absolute=False):
        """(M p) or (|M| p): camera rows A_c p_c + lam D p_c + E p_s, spline rows E^T p_c + band p_s + lam D p_s."""
        f = np.abs if absolute else (lambda a: a)
        yc = np.einsum('cij,cj->ci', f(self.A), pc.reshape(self.C, self.B)).reshape(-1) + self.damp_c * pc + f(self.E) @ ps
        P3 = ps.reshape(self.N, 3)
        y3 = np.zeros((self.N, 3), dtype=LD)
        for w in range(min(self.W, self.N)):
            blk = f(self.band[:self.N - w, w])
            y3[:self.N - w] += np.einsum('nij,nj->ni', blk, P3[w:])
            if w > 0:
                y3[w:] += np.einsum('nji,nj->ni', blk, P3[:self.N - w])          # the mirrored lower block
        ys = f(self.E).T @ pc + y3.reshape(-1) + self.damp_s * ps
        return yc, ys

    def norm_scaled_matrix(self):
        """|S M S|_inf: the largest absolute row sum, as s_i * (|M| s)_i."""
        yc, ys = self.matvec(self.sc, self.ss, absolute=True)
        return max(np.max(self.sc * yc), np.max(self.ss * ys))


def residual(prob, g, A, band, cross, lam, p):
    """r = M p + g in long double, x order, block by block."""
    s = _System(prob, g, A, band, cross, lam)
    yc, ys = s.matvec(*s.split(p))
    return s.join(yc + s.gc, ys + s.gs)


def eta(prob, g, A, band, cross, lam, p):
    """(eta, eta_cam, eta_spline): the scaled backward error of p, and the same quotient with the numerator restricted to the camera
    rows, respectively the spline rows (which half of the chain an excess came from).  Python floats."""
    s = _System(prob, g, A, band, cross, lam)
    pc, ps = s.split(p)
    yc, ys = s.matvec(pc, ps)
    rc, rs = np.max(np.abs(s.sc * (yc + s.gc))), np.max(np.abs(s.ss * (ys + s.gs)))
    size_p = max(np.max(np.abs(pc / s.sc)), np.max(np.abs(ps / s.ss)))
    size_g = max(np.max(np.abs(s.sc * s.gc)), np.max(np.abs(s.ss * s.gs)))
    den = s.norm_scaled_matrix() * size_p + size_g
    return Eta(float(max(rc, rs) / den), float(rc / den), float(rs / den))


def forward_scaled(prob, g, A, band, cross, lam, p, p_star):
    """|S^-1 (p - p*)|_inf / |S^-1 p*|_inf: the forward error in the units in which eta is a backward error."""
    s = _System(prob, g, A, band, cross, lam)
    pc, ps = s.split(p)
    qc, qs = s.split(p_star)
    num = max(np.max(np.abs((pc - qc) / s.sc)), np.max(np.abs((ps - qs) / s.ss)))
    return float(num / max(np.max(np.abs(qc / s.sc)), np.max(np.abs(qs / s.ss))))


def dense(prob, g, A, band, cross):
    """The dense H (n x n, x order, fp64) of the exported blocks, for the small cases."""
    n, C, B, N, W = int(prob.n_params), A.shape[0], A.shape[1], band.shape[0], band.shape[1]
    cam_idx, spl_idx = internal_index(prob)
    H = np.zeros((n, n))
    for c in range(C):
        H[np.ix_(cam_idx[c], cam_idx[c])] = A[c]
    E = cross.reshape(C * B, 3 * N)
    ci = cam_idx.ravel()
    H[np.ix_(ci, spl_idx)] = E
    H[np.ix_(spl_idx, ci)] = E.T
    for w in range(W):
        for gi in range(N - w):
            ri, cj = spl_idx[3 * gi:3 * gi + 3], spl_idx[3 * (gi + w):3 * (gi + w) + 3]
            H[np.ix_(ri, cj)] = band[gi, w]
            if w > 0:
                H[np.ix_(cj, ri)] = band[gi, w].T
    return H


def damped(H, lam):
    """M = H + lam * D of a dense H."""
    d = np.diag(H)
    return H + lam * np.diag(np.where(d > 0, d, 1.0))


def refined(prob, g, A, band, cross, lam):
    """p* in long double: a dense fp64 solve and four steps of iterative refinement with the long-double residual (n <= 1000)."""
    assert prob.n_params <= DENSE_MAX
    M = damped(dense(prob, g, A, band, cross), lam)
    p = -np.linalg.solve(M, g).astype(LD)
    for _ in range(4):
        r = residual(prob, g, A, band, cross, lam, p)
        p = p - np.linalg.solve(M, r.astype(np.float64)).astype(LD)
    return p


def kappa(prob, g, A, band, cross, lam, limit=DENSE_MAX):
    """cond_inf of the dense S M S (n <= 1000, unless the caller raises the limit for one system it knows)."""
    assert prob.n_params <= limit
    M = damped(dense(prob, g, A, band, cross), lam)
    s = 1.0 / np.sqrt(np.diag(M))
    return float(np.linalg.cond(M * np.outer(s, s), np.inf))


def blocks_from_dense(prob, H, grad):
    """A dense H (x order), cut into the blocks mvus_ba_normal_equations would export: (g, A, band, cross).  The band is as wide as
    the spline block needs (at least four control points); anything of H outside the three kinds of block is an error."""
    cam_idx, spl_idx = internal_index(prob)
    C, B, N = cam_idx.shape[0], cam_idx.shape[1], spl_idx.size // 3
    ci = cam_idx.ravel()
    A = np.stack([H[np.ix_(cam_idx[c], cam_idx[c])] for c in range(C)])
    Hc = H[np.ix_(ci, ci)].copy()
    for c in range(C):
        Hc[c * B:(c + 1) * B, c * B:(c + 1) * B] = 0
    assert not Hc.any(), 'cameras couple directly'
    Hs = H[np.ix_(spl_idx, spl_idx)]
    blocks = Hs.reshape(N, 3, N, 3).transpose(0, 2, 1, 3)
    i, j = np.nonzero(np.abs(blocks).max(axis=(2, 3)))
    W = max(4, int(np.max(np.abs(i - j))) + 1)
    band = np.zeros((N, W, 3, 3))
    for w in range(W):
        for gi in range(N - w):
            band[gi, w] = blocks[gi, gi + w]
    cross = H[np.ix_(ci, spl_idx)].reshape(C, B, 3 * N).copy()
    return np.array(grad, dtype=np.float64), A, band, cross
