"""Reference for the spline fit's band solvers (k_band_solve, k_band_solve_parts, k_band_diag_sum of mvus_amd/csrc/spline_band_solve*.hip.h,
reached through mvus_spline_band_solve / mvus_spline_band_diag_sum): seeded systems with a known factor, a banded Cholesky solve in
mpmath at 50 digits, and the list of cases tests/test_gpu_band_solve.py runs -- tests/test_band_solve_host.py asserts the premises of
every system on that list without a GPU.

Systems.  M = L0 L0^T at 50 digits, L0 lower banded with L0(j, j) = 10^(-D u_j), u_j uniform in [0, 1), and
L0(j, j - w) = U(-0.4, 0.4) L0(j - w, j - w): the Cholesky factor is unique, so L0 IS the natural-order factor and its diagonal spans D
decades by construction.  Families: A D = 0.5; B D = 2.5 (ratio 316, below the fit's 1e4 switch to double-double); C D = 5 (1e5: above
the switch, no pivot lost in fp64); D D = 8 (fp64 loses pivots, double-double does not); E = A with one row and column zeroed (a zero
diagonal entry: the kernels' pivot-of-one branch; the right-hand side is zeroed there too, the system stays consistent).  Every entry
and the three right-hand sides are split into a high and a low double.  The fp64 system is the high words taken exactly, the
double-double system is hi + lo taken exactly: the reference always solves exactly what the kernel was given.  With hb = 4 the entry
point forms G5 + pinv^2 BtB itself; M is handed over as G5 = M / 2 (w < 4; nothing at w = 4, as in a fit) and BtB = 2 M (4 M at w = 4)
with pinv = 1 / 2 -- powers of two, so the sum is M to the bit in either precision.  'G' is a genuine pair: A^T A and A^T X of a
seeded trajectory's design matrix, B^T B of FITPACK's jump matrix (fpdisc), both accumulated exactly from their fp64 factors.
"""
import functools
import math
from types import SimpleNamespace

import mpmath as mp
import numpy as np

DPS = 50
EPS = 2.0 ** -53
DECADES = {'A': 0.5, 'B': 2.5, 'C': 5.0, 'D': 8.0, 'E': 0.5}
GENUINE_PINV = (1.0 / 0.37, 1.0 / 25.0)                    # 1 / p for a small and a large smoothing parameter


def kbar(hb):
    """Higham's constant for a Cholesky solve whose factor rows have at most 2 hb + 1 entries: gamma_{3 (2 hb + 1) + 1}"""
    return 3 * (2 * hb + 1) + 1


# ---- the partition, restated (the host test holds it against the library's band_parts / band_parts_fixed) -------------------------
def parts_fixed(n, hb, P):
    """(len, rem) of P interiors, or None when an interior would be shorter than 2 hb rows"""
    inner = n - (P - 1) * hb
    if P < 2 or P > 256 or inner <= 0 or inner // P < 2 * hb:
        return None
    return inner // P, inner - (inner // P) * P


def parts_rule(n, hb, min_rows=192):
    """P of the production rule (1: one chain)"""
    if n < min_rows:
        return 1
    P = max(2, min(256, int(math.sqrt(n / 2.5))))
    while P > 1 and parts_fixed(n, hb, P) is None:
        P -= 1
    return max(P, 1)


def parts_order(n, hb, P):
    """rows in the elimination order of k_band_solve_parts: the interiors one after the other, then the separators"""
    ln, rem = parts_fixed(n, hb, P)
    inner, seps, j = [], [], 0
    for p in range(P):
        lp = ln + (1 if p < rem else 0)
        inner += range(j, j + lp)
        j += lp
        if p + 1 < P:
            seps += range(j, j + hb)
            j += hb
    assert j == n
    return np.array(inner + seps)


# ---- systems ------------------------------------------------------------------------------------------------------------------------
def _split(x):
    hi = float(x)
    return hi, float(x - mp.mpf(hi))


def _split_band(Mb, n):
    hi, lo = np.zeros((n, 5)), np.zeros((n, 5))
    for j in range(n):
        for w, v in enumerate(Mb[j]):
            hi[j, w], lo[j, w] = _split(v)
    return hi, lo


@functools.lru_cache(maxsize=None)
def synthetic(family, n, hb, seed=0):
    rng = np.random.default_rng([seed, n, hb, ord(family)])
    u, off = rng.random(n), rng.uniform(-0.4, 0.4, (n, hb))
    rhs = rng.standard_normal((3, n))
    rhs_lo = rhs * rng.uniform(-1, 1, (3, n)) * 2.0 ** -54
    with mp.workdps(DPS):
        d = [mp.power(10, -mp.mpf(DECADES[family]) * mp.mpf(float(x))) for x in u]
        L0 = [[d[j]] + [mp.mpf(float(off[j, w - 1])) * d[j - w] if j - w >= 0 else mp.mpf(0) for w in range(1, hb + 1)] for j in range(n)]
        Mb = [[mp.fsum(L0[j][v] * L0[j - w][v - w] for v in range(w, hb + 1) if j - v >= 0) if j - w >= 0 else mp.mpf(0)
               for w in range(hb + 1)] for j in range(n)]
        zeroed = None
        if family == 'E':
            zeroed = n // 2
            Mb[zeroed] = [mp.mpf(0)] * (hb + 1)
            for w in range(1, hb + 1):
                if zeroed + w < n:
                    Mb[zeroed + w][w] = mp.mpf(0)
            rhs[:, zeroed] = 0.0
            rhs_lo[:, zeroed] = 0.0
        hi, lo = _split_band(Mb, n)
    s = SimpleNamespace(family=family, n=n, hb=hb, rhs=rhs, rhs_lo=rhs_lo, zeroed=zeroed, name='%s n=%d hb=%d' % (family, n, hb),
                        L0_diag=[float(x) for x in d])
    if hb == 3:
        s.G5, s.G5_lo, s.BtB, s.BtB_lo, s.pinv = hi, lo, None, None, 0.0
    else:
        scale_g, scale_b = np.array([0.5, 0.5, 0.5, 0.5, 0.0]), np.array([2.0, 2.0, 2.0, 2.0, 4.0])
        s.G5, s.G5_lo, s.BtB, s.BtB_lo, s.pinv = hi * scale_g, lo * scale_g, hi * scale_b, lo * scale_b, 0.5
    return s


def fpdisc(t):
    """Dierckx's fpdisc for k = 3: row l of the jump matrix holds the discontinuity of the third derivative of B-splines l .. l + 4 at
    interior knot t[l + 4], scaled by ((n - 7) / (t[n - 4] - t[3]))^3 -- b[n - 8, 5]"""
    n, k, k1, k2 = len(t), 3, 4, 5
    nk1 = n - k1
    fac = (nk1 - k) / (t[nk1] - t[k1 - 1])
    b = np.zeros((max(0, n - 2 * k1), k2))
    for l in range(k2, nk1 + 1):
        lmk = l - k1
        h = np.zeros(2 * k1)
        for j in range(1, k1 + 1):
            h[j - 1] = t[l - 1] - t[l + j - k2 - 1]
            h[j + k1 - 1] = t[l - 1] - t[l + j - 1]
        lp = lmk
        for j in range(1, k2 + 1):
            prod = h[j - 1]
            for i in range(1, k + 1):
                prod = prod * h[j + i - 1] * fac
            b[lmk - 1, j - 1] = (t[lp + k1 - 1] - t[lp - 1]) / prod
            lp += 1
    return b


GENUINE_M, GENUINE_STEP = 2400, 3                          # 802 coefficients: 65 interiors of 8 rows fit with hb = 4


@functools.lru_cache(maxsize=None)
def genuine_operands():
    """knots, the exact A^T A, A^T X and B^T B (banded, mpmath) of a seeded trajectory with a knot at every third sample"""
    from scipy.interpolate import BSpline
    from test_traj_to_spline import _trajectory
    u, X = _trajectory(21, GENUINE_M, speed=3)
    t = np.concatenate(([u[0]] * 4, u[GENUINE_STEP:-GENUINE_STEP:GENUINE_STEP], [u[-1]] * 4))
    n = t.size - 4
    A = BSpline.design_matrix(u, t, 3).tocsr()
    b = fpdisc(t)
    with mp.workdps(DPS):
        G = [[mp.mpf(0)] * 5 for _ in range(n)]
        R = [[mp.mpf(0)] * n for _ in range(3)]
        for i in range(u.size):
            cols, vals = A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]
            for ca, va in zip(cols, vals):
                for cb, vb in zip(cols, vals):
                    if cb <= ca:
                        G[ca][ca - cb] += mp.mpf(float(va)) * mp.mpf(float(vb))
                for dim in range(3):
                    R[dim][ca] += mp.mpf(float(va)) * mp.mpf(float(X[dim, i]))
        B = [[mp.mpf(0)] * 5 for _ in range(n)]
        for it in range(b.shape[0]):
            for ca in range(5):
                for cb in range(ca + 1):
                    B[it + ca][ca - cb] += mp.mpf(float(b[it, ca])) * mp.mpf(float(b[it, cb]))
        G5, G5_lo = _split_band(G, n)
        BtB, BtB_lo = _split_band(B, n)
        rhs, rhs_lo = np.zeros((3, n)), np.zeros((3, n))
        for dim in range(3):
            for j in range(n):
                rhs[dim, j], rhs_lo[dim, j] = _split(R[dim][j])
    return SimpleNamespace(t=t, b=b, n=n, G5=G5, G5_lo=G5_lo, BtB=BtB, BtB_lo=BtB_lo, rhs=rhs, rhs_lo=rhs_lo)


@functools.lru_cache(maxsize=None)
def genuine(hb, which=0):
    g = genuine_operands()
    s = SimpleNamespace(family='G', n=g.n, hb=hb, G5=g.G5, G5_lo=g.G5_lo, rhs=g.rhs, rhs_lo=g.rhs_lo, zeroed=None, BtB=None, BtB_lo=None, pinv=0.0,
                        name='G n=%d hb=%d' % (g.n, hb))
    if hb == 4:
        s.BtB, s.BtB_lo, s.pinv = g.BtB, g.BtB_lo, GENUINE_PINV[which]
        s.name += ' pinv=%.3g' % s.pinv
    return s


def system(key):
    """key = (family, n, hb) or ('G', which, hb)"""
    return genuine(key[2], key[1]) if key[0] == 'G' else synthetic(*key)


# ---- the reference solve ------------------------------------------------------------------------------------------------------------
def _exact_band(s, precise):
    """the matrix the kernel is asked to solve, exactly: G5 + pinv^2 BtB on the high words (fp64) or on hi + lo (double-double)"""
    hb, n = s.hb, s.n
    p2 = mp.mpf(s.pinv) ** 2
    Mb = []
    for j in range(n):
        row = []
        for w in range(hb + 1):
            v = mp.mpf(float(s.G5[j, w])) + (mp.mpf(float(s.G5_lo[j, w])) if precise else 0)
            if s.BtB is not None:
                v += p2 * (mp.mpf(float(s.BtB[j, w])) + (mp.mpf(float(s.BtB_lo[j, w])) if precise else 0))
            row.append(v if j - w >= 0 else mp.mpf(0))
        Mb.append(row)
    return Mb


_refs = {}


def reference(key, precise):
    """Banded Cholesky M = L L^T and both substitutions at 50 digits, in the natural order.  A diagonal entry that is exactly 0 (family
    E) takes the pivot 1, as in the kernels; its row and column are 0, so that unknown is 0."""
    ck = (key, bool(precise))
    if ck in _refs:
        return _refs[ck]
    s = system(key)
    hb, n = s.hb, s.n
    with mp.workdps(DPS):
        Mb = _exact_band(s, precise)
        b = [[mp.mpf(float(s.rhs[d, j])) + (mp.mpf(float(s.rhs_lo[d, j])) if precise else 0) for j in range(n)] for d in range(3)]
        L = [[mp.mpf(0)] * (hb + 1) for _ in range(n)]
        y = [[mp.mpf(0)] * n for _ in range(3)]
        for j in range(n):
            row = L[j]
            for w in range(min(hb, j), 0, -1):
                v = Mb[j][w]
                for u2 in range(w + 1, min(hb, j) + 1):
                    v -= row[u2] * L[j - w][u2 - w]
                row[w] = v / L[j - w][0]
            dg = Mb[j][0] - mp.fsum(row[w] * row[w] for w in range(1, hb + 1))
            if Mb[j][0] == 0:
                dg = mp.mpf(1)
            if dg <= 0:                                    # (the high words of family D alone need not be positive definite)
                r = SimpleNamespace(key=key, precise=bool(precise), n=n, hb=hb, Mb=Mb, b=b, c=None, spd=False)
                _refs[ck] = r
                return r
            row[0] = mp.sqrt(dg)
            for d in range(3):
                y[d][j] = (b[d][j] - mp.fsum(row[w] * y[d][j - w] for w in range(1, min(hb, j) + 1))) / row[0]
        c = [[mp.mpf(0)] * n for _ in range(3)]
        for j in range(n - 1, -1, -1):
            for d in range(3):
                c[d][j] = (y[d][j] - mp.fsum(L[j + w][w] * c[d][j + w] for w in range(1, min(hb, n - 1 - j) + 1))) / L[j][0]
        diag = [L[j][0] for j in range(n)]
        ratio = [float(diag[j] ** 2 / Mb[j][0]) for j in range(n) if Mb[j][0] != 0]
        r = SimpleNamespace(key=key, precise=bool(precise), n=n, hb=hb, Mb=Mb, b=b, c=c, spd=True, c64=np.array([[float(v) for v in col] for col in c]),
                            diag=np.array([float(v) for v in diag]), diag_sum=float(mp.fsum(diag)), ratio_min=min(ratio), ratio_max=max(ratio),
                            diag_min=float(min(diag)), diag_max=float(max(diag)))
    _refs[ck] = r
    return r


def _matvec(Mb, hb, n, x):
    out = []
    for j in range(n):
        out.append(mp.fsum([Mb[j][w] * x[j - w] for w in range(min(hb, j) + 1)] + [Mb[j + w][w] * x[j + w] for w in range(1, min(hb, n - 1 - j) + 1)]))
    return out


def norm_inf(Mb, hb, n):
    return max(mp.fsum([abs(Mb[j][w]) for w in range(min(hb, j) + 1)] + [abs(Mb[j + w][w]) for w in range(1, min(hb, n - 1 - j) + 1)]) for j in range(n))


def backward_error(ref, c):
    """max over the columns of |b - M c|_inf / (|M|_inf |c|_inf + |b|_inf), evaluated at 50 digits for the doubles c[3, n]"""
    with mp.workdps(DPS):
        if not hasattr(ref, 'norm'):
            ref.norm = norm_inf(ref.Mb, ref.hb, ref.n)
        worst = mp.mpf(0)
        for d in range(3):
            x = [mp.mpf(float(v)) for v in c[d]]
            Mx = _matvec(ref.Mb, ref.hb, ref.n, x)
            res = max(abs(ref.b[d][j] - Mx[j]) for j in range(ref.n))
            worst = max(worst, res / (ref.norm * max(abs(v) for v in x) + max(abs(v) for v in ref.b[d])))
        return float(worst)


def forward_error(ref, c):
    """max over the columns of max |c - c_ref| / max |c_ref|"""
    with mp.workdps(DPS):
        worst = 0.0
        for d in range(3):
            err = max(abs(mp.mpf(float(c[d, j])) - ref.c[d][j]) for j in range(ref.n))
            worst = max(worst, float(err / max(abs(v) for v in ref.c[d])))
        return worst


def dense(key):
    """the fp64 system as a dense matrix (the high words; G5 + pinv^2 BtB in fp64, exact for the synthetic families)"""
    s = system(key)
    band = s.G5.copy() if s.BtB is None else s.G5 + (s.pinv * s.pinv) * s.BtB
    M = np.zeros((s.n, s.n))
    for w in range(s.hb + 1):
        idx = np.arange(w, s.n)
        M[idx, idx - w] = band[w:, w]
        M[idx - w, idx] = band[w:, w]
    return M


_kappas = {}


def kappa_inf(key):
    """|M|_inf |M^-1|_inf of the fp64 system, by np.linalg.inv (families A, B: kappa below 1e8)"""
    if key not in _kappas:
        M = dense(key)
        _kappas[key] = float(np.abs(M).sum(axis=1).max() * np.abs(np.linalg.inv(M)).sum(axis=1).max())
    return _kappas[key]


def kappa_inf_mp(ref):
    """the same at 50 digits, from the reference's own factor: one pair of banded substitutions per column of the inverse (small n only)"""
    n, hb = ref.n, ref.hb
    if hasattr(ref, 'kappa'):
        return ref.kappa
    with mp.workdps(DPS):
        Lb =[[mp.mpf(0)] * (hb + 1) for _ in range(n)]
        for j in range(n):
            row = Lb[j]
            for w in range(min(hb, j), 0, -1):
                v = ref.Mb[j][w]
                for u2 in range(w + 1, min(hb, j) + 1):
                    v -= row[u2] * Lb[j - w][u2 - w]
                row[w] = v / Lb[j - w][0]
            row[0] = mp.sqrt(ref.Mb[j][0] - mp.fsum(row[w] * row[w] for w in range(1, hb + 1)))
        rowsum = [mp.mpf(0)] * n
        for e in range(n):
            y = [mp.mpf(0)] * n
            for j in range(e, n):
                y[j] = ((1 if j == e else 0) - mp.fsum(Lb[j][w] * y[j - w] for w in range(1, min(hb, j) + 1))) / Lb[j][0]
            x = [mp.mpf(0)] * n
            for j in range(n - 1, -1, -1):
                x[j] = (y[j] - mp.fsum(Lb[j + w][w] * x[j + w] for w in range(1, min(hb, n - 1 - j) + 1))) / Lb[j][0]
                rowsum[j] += abs(x[j])                     # column e of the symmetric inverse = row e
        ref.kappa = float(norm_inf(ref.Mb, hb, n) * max(rowsum))
        return ref.kappa


def permuted_diag(key, P):
    """diag of the fp64 dense Cholesky factor of the permuted matrix (interiors in order, then separators in order): block elimination
    IS that Cholesky, so these are the pivots of k_band_solve_parts"""
    s = system(key)
    order = parts_order(s.n, s.hb, P)
    M = dense(key)
    return np.linalg.cholesky(M[np.ix_(order, order)]).diagonal()


# ---- the cases of tests/test_gpu_band_solve.py ------------------------------------------------------------------------------------------
CHAIN_N = (4, 5, 8, 63, 64, 65, 191)
DIAG_N = (4, 63, 64, 65, 128, 129, 200)
BIG_P = (63, 64, 65, 128, 129, 256)
SUBSET_N = 800                                             # families B, C, E: one chain, P = 2, P = 3 and P = 65 on one system per hb
SMALL_D_N = 120                                            # family D: a system whose kappa is affordable at 50 digits (and SUBSET_N for P = 65)


def parts_shapes(hb):
    """(n, parts, what) of family A: the smallest shapes at which each path of k_band_solve_parts can go wrong"""
    out = [(5 * hb, 2, 'P=2 shortest'), (5 * hb + 1, 2, 'P=2 one row more'), (8 * hb, 3, 'P=3 first W')]
    if hb == 3:
        out.append((2 * 7 + hb, 2, 'interiors of 7 rows'))
    for ln in (8, 9, 16, 17):
        out.append((3 * ln + 2 * hb, 3, 'interiors of %d rows' % ln))
    for extra in (0, 1, 4):
        out.append((5 * (2 * hb + 2) + 4 * hb + extra, 5, 'P=5 rem=%d' % extra))
    for P in BIG_P:
        n0 = P * 2 * hb + (P - 1) * hb
        out += [(n0, P, 'P=%d interiors of 2hb' % P), (n0 + P - 1, P, 'P=%d interiors of 2hb+1, rem=P-1' % P)]
    out += [(192, 0, 'rule, first partitioned'), (191, 0, 'rule, last chain'), (700, 0, 'rule')]
    return [s for k, s in enumerate(out) if s[:2] not in [o[:2] for o in out[:k]]]      # (hb = 4: 'first W' already has interiors of 8 rows)


def solve_cases():
    """(key, parts) of every mvus_spline_band_solve case; each runs in fp64 and in double-double"""
    cases = []
    for hb in (3, 4):
        cases += [(('A', n, hb), -1) for n in CHAIN_N]
        cases += [(('A', n, hb), parts) for n, parts, _ in parts_shapes(hb)]
        for fam in 'BCE':
            cases += [((fam, SUBSET_N, hb), parts) for parts in (-1, 2, 3, 65)]
        cases += [(('D', SMALL_D_N, hb), parts) for parts in (-1, 2, 3)] + [(('D', SUBSET_N, hb), 65)]     # (65 interiors do not fit 200 rows)
    cases += [(('G', 0, 3), parts) for parts in (-1, 2, 3, 65, 0)]
    for which in (0, 1):
        cases += [(('G', which, 4), parts) for parts in (-1, 2, 3, 65, 0)]
    return cases


def diag_cases():
    return [('A', n, 3) for n in DIAG_N] + [(fam, SUBSET_N, 3) for fam in 'BC'] + [('G', 0, 3)]


def all_keys():
    seen = []
    for key in [k for k, _ in solve_cases()] + diag_cases():
        if key not in seen:
            seen.append(key)
    return seen


def case_id(key, parts=None, precise=None):
    s = '%s-%s-hb%d' % (key[0], ('pinv%d' % key[1]) if key[0] == 'G' else ('n%d' % key[1]), key[2])
    if parts is not None:
        s += '-chain' if parts == -1 else ('-rule' if parts == 0 else '-P%d' % parts)
    if precise is not None:
        s += '-dd' if precise else '-fp64'
    return s
