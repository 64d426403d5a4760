"""Reference for the passes of the smoothing fit around its band solvers (k_fit_basis, k_fit_first, k_fit_blocks, k_fit_slice_sum,
k_fit_band, k_fit_penalty, k_fit_residual, k_fit_total_partial / k_fit_total, k_fit_fpint / k_fit_fpint_final of
mvus_amd/csrc/spline_fit_passes.hip.h, reached through mvus_spline_fit_normal / _penalty / _residual): exact sums in rational arithmetic of
exactly what a kernel was given, the basis by de Boor's recurrence at 50 digits, and the list of cases tests/test_gpu_fit_passes.py runs.
Host only: nothing here comes from the GPU; tests/test_fit_passes_host.py asserts the premises of every case and holds this module to
scipy and to oracle/fitpack_oracle.py.

Chain lengths (the k of a bar k * unit * sum |terms|) are counted from the launches:
  a block of k_fit_blocks<T, NT> over `count` samples in `slices` slices: per = ceil(count / slices) samples a workgroup, so
  ceil(per / NT) serial additions a thread, log2 NT levels of block_sum's tree, slices - 1 additions in k_fit_slice_sum;
  an entry of G5 / rhs adds up to 4 such blocks (3 additions, k_fit_band) and every term is one rounded product: + 3 + 1;
  NT = 256 in fp64 and 64 in double-double; the unit is 2^-53 / 2^-100 (tests/test_gpu_band_solve.py's convention);
  an entry of B^T B is at most 5 products: k = 6;
  the total: ceil(m / 256) + 8 in one stage; ceil(m / (256 nbt)) + 8, then ceil(nbt / 256) + 8 in two (nbt = fit_total_parts(m));
  a per-span residual: ceil(per / 256) + 8, slices - 1 more in k_fit_fpint_final, and the two halves (+ 3 with the bar's own + 1)."""
import functools
import math
from bisect import bisect_left, bisect_right
from fractions import Fraction
from types import SimpleNamespace

import mpmath
import numpy as np

EPS = 2.0 ** -53
U100 = 2.0 ** -100
KQ = 15                       # roundings on the longest path of bspline_basis_w<false>: 5 a level (see basis_bar)
K_FIT_BLK = 22
K_SLICE_BLOCKS = 1536
TOTAL_ONE_STAGE = 8192
TOTAL_PARTS = 1024


def gamma(k, unit=EPS):
    return k * unit / (1 - k * unit)


# ---- the rules restated ---------------------------------------------------------------------------------------------------------------
def fit_slices(nspan):
    return 1 if nspan >= 512 else min(256, (1024 + nspan - 1) // nspan)


def slices_legal(nspan, slices):
    return 1 <= slices <= 256 and nspan * (slices - 1) <= K_SLICE_BLOCKS and (slices == 1 or nspan * slices <= 512 + K_SLICE_BLOCKS)


def total_parts(m):
    return min(TOTAL_PARTS, (m + 2047) // 2048)


def exact_first(u, t):
    """first[sp] = the first index with u >= t[3 + sp], first[0] = 0, first[nspan] = m: comparisons on the doubles"""
    n, m = len(t), len(u)
    nspan = n - 7
    ul = [float(v) for v in u]
    return np.array([0] + [bisect_left(ul, float(t[3 + sp])) for sp in range(1, nspan)] + [m], dtype=np.int64)


def exact_span(u, t):
    """FITPACK's span: t[3 + sp] <= u < t[4 + sp], the last sample in the last span"""
    n = len(t)
    interior = [float(v) for v in t[4:n - 4]]
    return np.array([min(bisect_right(interior, float(x)), n - 8) for x in u], dtype=np.int32)


def basis50(u, t, span=None):
    """the four cubic B-splines of every sample on its span, de Boor's recurrence at 50 digits on the double inputs: list of 4 mpf a sample"""
    span = exact_span(u, t) if span is None else span
    out = []
    with mpmath.workdps(50):
        tm = [mpmath.mpf(float(v)) for v in t]
        for x, sp in zip(u, span):
            l, x = int(sp) + 3, mpmath.mpf(float(x))
            h = [mpmath.mpf(1), mpmath.mpf(0), mpmath.mpf(0), mpmath.mpf(0)]
            for j in range(1, 4):
                hh = h[:j]
                h[0] = mpmath.mpf(0)
                for i in range(j):
                    tli, tlj = tm[l + i + 1], tm[l + i + 1 - j]
                    f = hh[i] / (tli - tlj)
                    h[i] = h[i] + f * (tli - x)
                    h[i + 1] = f * (x - tlj)
            out.append(h)
    return out


def basis_errors(q, ref):
    """largest relative error of q[m, 4] against basis50's values, and whether every exact zero is a zero (and nothing else is)"""
    worst, zeros_ok = 0.0, True
    with mpmath.workdps(50):
        for row, hr in zip(q, ref):
            for a in range(4):
                if hr[a] == 0:
                    zeros_ok &= float(row[a]) == 0.0
                else:
                    zeros_ok &= float(row[a]) != 0.0
                    worst = max(worst, float(abs(mpmath.mpf(float(row[a])) - hr[a]) / abs(hr[a])))
    return worst, zeros_ok


def basis_bar():
    """Every value of a level is f (tli - x) or a sum of two such non-negative products, f = hh / (tli - tlj): it inherits the relative
    error of hh and adds one rounding each for the knot difference, the division, tli - x (or x - tlj), the product and the sum -- 5 a
    level, 3 levels (fused products only remove roundings).  No cancellation: every term is >= 0 on the sample's own span."""
    return gamma(KQ)


# ---- exact accumulation -------------------------------------------------------------------------------------------------------------
def _fr(a):
    return [Fraction(float(v)) for v in a]


def exact_blocks(q, X, first):
    """per span: (sum, sum of |terms|) of the 22 products of k_fit_blocks over samples first[sp] .. first[sp + 1] - 1, from the given q"""
    m = q.shape[0]
    qf = [_fr(q[i]) for i in range(m)]
    xf = [_fr(X[:, i]) for i in range(m)]
    blocks = []
    for sp in range(len(first) - 1):
        s, sa = [Fraction(0)] * K_FIT_BLK, [Fraction(0)] * K_FIT_BLK
        for i in range(int(first[sp]), int(first[sp + 1])):
            h, x = qf[i], xf[i]
            for a in range(4):
                for b in range(a + 1):
                    p = h[a] * h[b]
                    s[a * (a + 1) // 2 + b] += p
                    sa[a * (a + 1) // 2 + b] += abs(p)
                for d in range(3):
                    p = h[a] * x[d]
                    s[10 + 3 * a + d] += p
                    sa[10 + 3 * a + d] += abs(p)
        blocks.append((s, sa))
    return blocks


def block_chain(count, slices, NT):
    per = -(-count // slices)
    return -(-per // NT) + int(math.log2(NT)) + (slices - 1)


def exact_normal(q, X, first, slices, NT, blocks=None):
    """G5[ncoef][5], rhs[3][ncoef] as k_fit_band assembles them from the exact blocks: per entry (value, sum |terms|, chain length)"""
    blocks = exact_blocks(q, X, first) if blocks is None else blocks
    nspan = len(blocks)
    ncoef = nspan + 3
    chain = [block_chain(int(first[sp + 1] - first[sp]), slices, NT) for sp in range(nspan)]
    zero = (Fraction(0), Fraction(0), 0)
    G5 = [[zero] * 5 for _ in range(ncoef)]
    rhs = [[zero] * ncoef for _ in range(3)]
    for j in range(ncoef):
        sps = range(max(0, j - 3), min(nspan - 1, j) + 1)
        k = max(chain[sp] for sp in sps) + 3 + 1
        for w in range(4):
            idx = [(sp, (j - sp) * (j - sp + 1) // 2 + (j - sp - w)) for sp in sps if j - sp - w >= 0]
            G5[j][w] = (sum(blocks[sp][0][e] for sp, e in idx), sum(blocks[sp][1][e] for sp, e in idx), k)
        for d in range(3):
            rhs[d][j] = (sum(blocks[sp][0][10 + 3 * (j - sp) + d] for sp in sps), sum(blocks[sp][1][10 + 3 * (j - sp) + d] for sp in sps), k)
    return G5, rhs


def exact_btb(b, ncoef):
    """(B^T B)(j, j - w) for the jump matrix b[n8, 5] (row it: columns it .. it + 4): per entry (value, sum |terms|)"""
    n8 = b.shape[0]
    bf = [_fr(r) for r in b]
    out = [[(Fraction(0), Fraction(0))] * 5 for _ in range(ncoef)]
    for j in range(ncoef):
        for w in range(5):
            terms = [bf[it][j - it] * bf[it][j - it - w] for it in range(max(0, j - 4), min(n8 - 1, j) + 1) if j - it - w >= 0]
            out[j][w] = (sum(terms, Fraction(0)), sum((abs(v) for v in terms), Fraction(0)))
    return out


def exact_term(q, c, X, span):
    """term[i] = sum_d (sum_a c[d, span + a] q[i, a] - X[d, i])^2 as rationals, and the bar of k_fit_residual for it:
    delta_d = gamma_5 (sum |c q| + |x_d|) bounds the error of r_d (4 products, 3 + 1 additions), so the error of the sum of squares is at most
    sum_d (2 |r_d| delta_d + delta_d^2) + gamma_4 term (three squares, two additions and one to spare)"""
    m = q.shape[0]
    ncoef = c.shape[1]
    cf = [_fr(c[d]) for d in range(3)]
    terms, bars = [], []
    g5, g4 = gamma(5), gamma(4)
    for i in range(m):
        h, sp = _fr(q[i]), int(span[i])
        assert 0 <= sp <= ncoef - 4
        tot, bar = Fraction(0), 0.0
        for d in range(3):
            prods = [cf[d][sp + a] * h[a] for a in range(4)]
            x = Fraction(float(X[d, i]))
            r = sum(prods) - x
            delta = g5 * float(sum(abs(p) for p in prods) + abs(x))
            bar += 2 * abs(float(r)) * delta + delta * delta
            tot += r * r
        terms.append(tot)
        bars.append(bar + g4 * float(tot))
    return terms, np.array(bars)


def fpint_closed(term, first):
    """the closed rule: the samples strictly inside a span, half of the sample that opens it, half of the one that opens the next span"""
    nspan = len(first) - 1
    tf = term if isinstance(term[0], Fraction) else _fr(term)
    out = []
    for sp in range(nspan):
        a, b = int(first[sp]), int(first[sp + 1])
        s = sum(tf[a + (1 if sp > 0 else 0):b], Fraction(0))
        if sp > 0:
            s += tf[a] / 2
        if sp + 1 < nspan:
            s += tf[b] / 2
        out.append(s)
    return out


def fpint_fppara(term, u, t):
    """fppara's loop over the samples, line by line (`new`, `store`, `fpart`; 1-based l kept), in rational arithmetic on the given term"""
    n, m = len(t), len(u)
    k1, k2 = 4, 5
    nk1 = n - k1
    nrint = nk1 - 3
    tf = term if isinstance(term[0], Fraction) else _fr(term)
    fpint = [Fraction(0)] * nrint
    fpart, i, l, new = Fraction(0), 1, k2, 0
    for it in range(1, m + 1):
        if not (float(u[it - 1]) < float(t[l - 1]) or l > nk1):
            new = 1
            l = l + 1
        tm = tf[it - 1]
        fpart = fpart + tm
        if new == 0:
            continue
        store = tm / 2
        fpint[i - 1] = fpart - store
        i = i + 1
        fpart = store
        new = 0
    fpint[nrint - 1] = fpart
    return fpint


def total_chain(m):
    if m > TOTAL_ONE_STAGE:
        nbt = total_parts(m)
        return -(-m // (256 * nbt)) + 8 + -(-nbt // 256) + 8
    return -(-m // 256) + 8


def fpint_chain(first, slices):
    nspan = len(first) - 1
    return [-(-(-(-max(int(first[sp + 1] - first[sp]) - (1 if sp > 0 else 0), 0) // slices)) // 256) + 8 + (slices - 1) for sp in range(nspan)]


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def samples(m, seed):
    """seeded, non-uniform timestamps (cumulative U(0.2, 1.8)) and a smooth curve of size about 10 plus noise"""
    rng = np.random.default_rng(seed)
    u = np.cumsum(rng.uniform(0.2, 1.8, m))
    s = u / u[-1]
    X = np.stack([10 * np.cos(3 * s) + 2 * s, 8 * np.sin(2.5 * s + 0.3), 6 * s * s - 4 * np.cos(5 * s)]) + 0.05 * rng.standard_normal((3, m))
    return u, X


def knots(u, interior):
    return np.concatenate(([u[0]] * 4, np.asarray(interior, dtype=np.float64), [u[-1]] * 4))


def _case(name, m, interior, configs, seed=None, single=(), note=''):
    """interior: function of u -> interior knots; configs: [(slices, parts)] (0: the production rule); single: spans holding one sample"""
    return SimpleNamespace(name=name, m=m, interior=interior, configs=configs, seed=seed if seed is not None else 1000 + m, single=tuple(single), note=note)


def _every_other(nspan):
    return lambda u: u[2:2 * nspan:2]


def normal_cases():
    cs = []
    for m in (4, 5, 63, 64, 65, 255, 256, 257):
        cs.append(_case('one-m%d' % m, m, lambda u: [], [(0, 0)]))
    cs.append(_case('one-m600', 600, lambda u: [], [(0, 0), (1, 0), (2, 0), (3, 0), (7, 0)]))
    cs.append(_case('two-left1', 40, lambda u: [u[1]], [(0, 0), (1, 0)], single=(0,)))
    cs.append(_case('two-right2', 40, lambda u: [u[-2]], [(0, 0), (1, 0)]))
    cs.append(_case('three-1-2-2997', 3000, lambda u: [u[1], u[3]], [(0, 0), (1, 0), (2, 0), (256, 0)], single=(0,)))
    cs.append(_case('interp-m12', 12, lambda u: u[2:-2], [(0, -1), (0, 0)], single=tuple(range(1, 8))))
    cs.append(_case('interp-m300', 300, lambda u: u[2:-2], [(0, -1), (0, 0), (0, 2)], single=tuple(range(1, 296))))
    cs.append(_case('off-mid', 50, lambda u: [(u[k] + u[k + 1]) / 2 for k in (5, 12, 13, 30, 44)], [(0, 0), (1, 0)], single=(2,)))
    cs.append(_case('off-above', 50, lambda u: [u[10], np.nextafter(u[20], np.inf), u[35]], [(0, 0), (1, 0)]))
    cs.append(_case('off-below', 50, lambda u: [u[10], np.nextafter(u[20], -np.inf), u[35]], [(0, 0), (1, 0)]))
    cs.append(_case('off-last', 50, lambda u: [u[10], u[30], np.nextafter(u[-2], -np.inf)], [(0, 0), (1, 0)]))
    for ncoef in (255, 256, 257):
        cs.append(_case('edge-ncoef%d' % ncoef, 2 * ncoef, _every_other(ncoef - 3), [(0, 0)]))
    for nspan in (511, 512):
        cs.append(_case('edge-nspan%d' % nspan, 1100, _every_other(nspan), [(0, 0)], seed=77))
    return cs


def total_cases():
    """residual only: the switch between the one-stage and the two-stage total"""
    return [_case('total-m8192', 8192, lambda u: [u[100], u[4000]], [(0, 0)]), _case('total-m8193', 8193, lambda u: [u[100], u[4000]], [(0, 0)])]


BIG_M = 2_100_000


@functools.lru_cache(maxsize=None)
def build(name):
    c = {c.name: c for c in normal_cases() + total_cases()}[name]
    u, X = samples(c.m, c.seed)
    t = knots(u, c.interior(u))
    return SimpleNamespace(case=c, u=u, X=X, t=t, n=t.size, ncoef=t.size - 4, nspan=t.size - 7, first=exact_first(u, t), span=exact_span(u, t))


def coefficient_sets(ncoef, seed):
    """random coefficients of the curve's size, and zero (the least-squares solution is the third set: it comes from the device)"""
    rng = np.random.default_rng(seed)
    return {'random': 10 * rng.standard_normal((3, ncoef)), 'zero': np.zeros((3, ncoef))}


def penalty_cases():
    """(name, ncoef, b): b from oracle/fitpack_oracle.fpdisc on seeded non-uniform knots for n8 = ncoef - 4 rows, and one random b with
    magnitudes spread over 1e-8 .. 1e8"""
    from oracle import fitpack_oracle as fo
    out = []
    for ncoef in (5, 6, 7, 8, 9, 10, 255, 256, 257):
        n = ncoef + 4
        rng = np.random.default_rng(500 + ncoef)
        inner = np.cumsum(rng.uniform(0.2, 1.8, n - 7))
        t = np.concatenate(([0.0] * 4, inner[:-1], [inner[-1]] * 4))
        out.append(('fpdisc-n8=%d' % (n - 8), ncoef, fo.fpdisc(t, n, 5)))
    rng = np.random.default_rng(9)
    out.append(('random-spread', 40, rng.standard_normal((36, 5)) * 10.0 ** rng.uniform(-8, 8, (36, 5))))
    return out
