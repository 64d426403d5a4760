"""LSMR (Fong & Saunders 2011; the algorithm of scipy.sparse.linalg.lsmr, damping and norm estimates included) in plain numpy, on a dense
matrix and in a chosen number format: the yardstick of tests/test_lsmr_host.py and tests/test_gpu_lsmr.py.

    A = [J diag(D); diag(E)],  right-hand side [b; 0],  min |A x - [b; 0]|^2 + damp^2 |x|^2,  x_0 = 0

``dtype``: np.float64, np.longdouble (the reference: 64 mantissa bits on x86) or 'mp' -- mpmath numbers at mpmath.mp.dps digits in object
arrays, the same statements run at 50 digits.  The run never stops by itself: it makes exactly ``k`` iterations and records, after each
one, the iterate, the norm estimates and the quantity of every stopping test together with the istop scipy's rules would give for the
tolerances passed in (0 = go on), so a caller can read off where a run with those tolerances ends.
"""
from types import SimpleNamespace

import numpy as np


def _is_mp(dtype):
    return isinstance(dtype, str) and dtype == 'mp'


def cast(a, dtype):
    """array (or scalar) in the reference's number format"""
    if _is_mp(dtype):
        import mpmath
        a = np.asarray(a)
        out = np.empty(a.shape, dtype=object)
        flat = out.reshape(-1)
        for i, v in enumerate(np.asarray(a, dtype=np.float64).reshape(-1)):
            flat[i] = mpmath.mpf(float(v))
        return out if a.ndim else flat[0]
    return np.asarray(a, dtype=dtype) if np.ndim(a) else dtype(a)


def _sqrt(v):
    if isinstance(v, (float, np.floating)):
        return np.sqrt(v)
    import mpmath
    return mpmath.sqrt(v)


def _norm(v):
    return _sqrt(v @ v)


def _sgn(a):
    return int(a > 0) - int(a < 0)


def _sym_ortho(a, b):
    """scipy.sparse.linalg._isolve.lsmr._sym_ortho"""
    if b == 0:
        return _sgn(a) * (a * 0 + 1), a * 0, abs(a)
    if a == 0:
        return a * 0, _sgn(b) * (b * 0 + 1), abs(b)
    if abs(b) > abs(a):
        tau = a / b
        s = _sgn(b) / _sqrt(1 + tau * tau)
        c = s * tau
        r = b / s
    else:
        tau = b / a
        c = _sgn(a) / _sqrt(1 + tau * tau)
        s = c * tau
        r = a / c
    return c, s, r


def dense_operator(J, D=None, E=None, dtype=np.longdouble):
    """A = [J diag(D); diag(E)] as a dense array of ``dtype`` (J: the float64 Jacobian, every entry exact in the wider formats)."""
    A = cast(J, dtype)
    if D is not None:
        A = A * cast(D, dtype)[None, :]
    if E is not None:
        n = A.shape[1]
        bottom = cast(np.zeros((n, n)), dtype)
        Ed = cast(E, dtype)
        for i in range(n):
            bottom[i, i] = Ed[i]
        A = np.concatenate((A, bottom), axis=0)
    return A


def lsmr_iterates(A, b, damp=0.0, k=4, dtype=np.longdouble, atol=0.0, btol=0.0, conlim=0.0):
    """Exactly ``k`` iterations (fewer only where scipy returns before its loop, or the bidiagonalisation breaks down with an exact zero).
    A: dense, already of ``dtype`` (dense_operator); b: the top m entries of the right-hand side (zeros are appended for the rows of E).
    Returns a list with one record per iteration: itn, x (a copy), normr, normar, normA, condA, normx, test1, test2, test3, t1, rtol and
    istop -- what scipy's rules give there with (atol, btol, conlim) and no iteration limit."""
    rows, n = A.shape
    zero = cast(0.0, dtype)
    one = zero + 1
    u = cast(np.zeros(rows), dtype)
    u[:len(b)] = cast(b, dtype)
    damp, atol, btol = cast(damp, dtype), cast(atol, dtype), cast(btol, dtype)
    ctol = 1 / cast(conlim, dtype) if conlim > 0 else zero
    At = A.T.copy()
    normb = _norm(u)
    x = cast(np.zeros(n), dtype)
    beta = normb
    if beta > 0:
        u = u * (1 / beta)
        v = At @ u
        alpha = _norm(v)
    else:
        v = cast(np.zeros(n), dtype)
        alpha = zero
    if alpha > 0:
        v = v * (1 / alpha)
    zetabar = alpha * beta
    alphabar = alpha
    rho = rhobar = cbar = one
    sbar = zero
    h = v.copy()
    hbar = cast(np.zeros(n), dtype)
    betadd = beta
    betad = zero
    rhodold = one
    tautildeold = thetatilde = zeta = d = zero
    normA2 = alpha * alpha
    maxrbar = zero
    minrbar = cast(1e100, dtype)
    out = []
    if alpha * beta == 0:
        return out
    for itn in range(1, k + 1):
        u = A @ v - alpha * u
        beta = _norm(u)
        if beta > 0:
            u = u * (1 / beta)
            v = At @ u - beta * v
            alpha = _norm(v)
            if alpha > 0:
                v = v * (1 / alpha)
        chat, shat, alphahat = _sym_ortho(alphabar, damp)
        rhoold = rho
        c, s, rho = _sym_ortho(alphahat, beta)
        thetanew = s * alpha
        alphabar = c * alpha
        rhobarold = rhobar
        zetaold = zeta
        thetabar = sbar * rho
        rhotemp = cbar * rho
        cbar, sbar, rhobar = _sym_ortho(cbar * rho, thetanew)
        zeta = cbar * zetabar
        zetabar = -sbar * zetabar
        hbar = h - (thetabar * rho / (rhoold * rhobarold)) * hbar
        x = x + (zeta / (rho * rhobar)) * hbar
        h = v - (thetanew / rho) * h
        betaacute = chat * betadd
        betacheck = -shat * betadd
        betahat = c * betaacute
        betadd = -s * betaacute
        thetatildeold = thetatilde
        ctildeold, stildeold, rhotildeold = _sym_ortho(rhodold, thetabar)
        thetatilde = stildeold * rhobar
        rhodold = ctildeold * rhobar
        betad = -stildeold * betad + ctildeold * betahat
        tautildeold = (zetaold - thetatildeold * tautildeold) / rhotildeold
        taud = (zeta - thetatilde * tautildeold) / rhodold
        d = d + betacheck * betacheck
        normr = _sqrt(d + (betad - taud) * (betad - taud) + betadd * betadd)
        normA2 = normA2 + beta * beta
        normA = _sqrt(normA2)
        normA2 = normA2 + alpha * alpha
        maxrbar = max(maxrbar, rhobarold)
        if itn > 1:
            minrbar = min(minrbar, rhobarold)
        condA = max(maxrbar, rhotemp) / min(minrbar, rhotemp)
        normar = abs(zetabar)
        normx = _norm(x)
        test1 = normr / normb
        test2 = normar / (normA * normr) if normA * normr != 0 else cast(np.inf, dtype)
        test3 = 1 / condA
        t1 = test1 / (1 + normA * normx / normb)
        rtol = btol + atol * normA * normx / normb
        istop = 0
        if 1 + test3 <= 1:
            istop = 6
        if 1 + test2 <= 1:
            istop = 5
        if 1 + t1 <= 1:
            istop = 4
        if test3 <= ctol:
            istop = 3
        if test2 <= atol:
            istop = 2
        if test1 <= rtol:
            istop = 1
        out.append(SimpleNamespace(itn=itn, x=x.copy(), normr=normr, normar=normar, normA=normA, condA=condA, normx=normx,
                                   test1=test1, test2=test2, test3=test3, t1=t1, rtol=rtol, atol=atol, ctol=ctol, istop=istop))
        if beta == 0 or alpha == 0:
            break
    return out


def rel_dev(x, x_ref):
    """|x - x_ref|_2 / |x_ref|_2 in the reference's format, as a float"""
    xr = np.asarray(x_ref)
    if xr.dtype == object:
        d = np.array([xi - float(v) for xi, v in zip(xr, np.asarray(x, dtype=np.float64))], dtype=object)
        return float(_norm(d) / _norm(xr))
    d = np.asarray(x, dtype=xr.dtype) - xr
    return float(_norm(d) / _norm(xr))


NORMS = ('normr', 'normar', 'normA', 'condA')


def norms_dev(got, ref, which=NORMS):
    """largest relative deviation of the norm estimates ``which`` of ``got`` (default: normr, normar, normA, condA) from the record ``ref``"""
    return max(abs(float((type(getattr(ref, k))(getattr(got, k)) - getattr(ref, k)) / getattr(ref, k))) for k in which)
