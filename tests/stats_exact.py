"""The log-likelihood of the statistical stage evaluated with mpmath at 80 digits, written from tests/stats_model.py and the
R lines it cites (file:line of mapdamage/r/stats/): what tools/make_stats_exact.py stores in
tests/golden/stats_loglik_exact.npz.  Needs mpmath; the tests that only read the fixture do not import this module.

Every input is taken as the double it is (``mpf(float)`` is exact), so the value is the true likelihood of the very numbers
the device and the numpy restatement are given, not of nearby decimals."""

import mpmath
from mpmath import mp, mpf

import stats_model as M

DIGITS = 80
AGREE = mpf(10) ** -60           # the two ways to exp(Q) below, entry by entry


def _mp(x):
    return mpf(float(x))


def pmat_closed(tmu, rho, acgt, jukes_cantor=False):
    """exp(Q) for the Q of qmatHKY85 (function.r:50-64) in the closed form csrc/mdx_stats.hip uses; jukesCantorPmat2
    (function.r:44-48).  Rows = the base substituted."""
    if jukes_cantor:
        e = mpmath.exp(-tmu)
        return [[(mpf(1) / 4 - e / 4) + (e if i == j else 0) for j in range(4)] for i in range(4)]
    s = sum(acgt)
    out = [[None] * 4 for _ in range(4)]
    for j in range(4):
        pj, big = acgt[j], acgt[j] + acgt[j ^ 2]
        e1 = mpmath.exp(-tmu * rho * s)
        e2 = mpmath.exp(-tmu * (big + rho * (s - big)))
        base = pj + pj * (s / big - 1) * e1
        for i in range(4):
            if (i ^ j) & 1:
                out[i][j] = pj * (1 - e1) / s
            elif i == j:
                out[i][j] = (base + (big - pj) * s / big * e2) / s
            else:
                out[i][j] = (base - pj * s / big * e2) / s
    return out


def pmat_expm(tmu, rho, acgt):
    """The same matrix as the exponential of Q itself (function.r:50-64, getPmat's eigen() replaced by expm)."""
    rate = [[0, rho, 1, rho], [rho, 0, rho, 1], [1, rho, 0, rho], [rho, 1, rho, 0]]
    q = mpmath.matrix(4, 4)
    for i in range(4):
        for j in range(4):
            q[i, j] = tmu * rate[i][j] * acgt[j]
        q[i, i] = -sum(tmu * rate[i][j] * acgt[j] for j in range(4))
    e = mpmath.expm(q)
    return [[e[i, j] for j in range(4)] for i in range(4)]


def pmat(tmu, rho, acgt, jukes_cantor=False):
    closed = pmat_closed(tmu, rho, acgt, jukes_cantor)
    if not jukes_cantor:
        other = pmat_expm(tmu, rho, acgt)
        assert all(abs(closed[i][j] - other[i][j]) < AGREE for i in range(4) for j in range(4))
    return closed


def dnbinom_parts(x, size, prob):
    """The five summands of log dnbinom (seqProbVecLambda, function.r:76), or None at the point masses."""
    if prob == 1 or size == 0:
        return None
    return (mpmath.loggamma(x + size), -mpmath.loggamma(size), -mpmath.loggamma(x + 1), size * mpmath.log(prob),
            x * mpmath.log1p(-prob))


def side(lam, disp, n):
    """psum[j] = (1 - cumsum(dnbinom(0..j))) / 2 (function.r:74-88) for j < n, and W[j] = sum_{q <= j} pv[q] A_q / 2 with
    A_q the sum of the magnitudes of log dnbinom's summands: how far an error of one ulp in each of them moves psum[j]."""
    psum, weight, c, w = [], [], mpf(0), mpf(0)
    for q in range(n):
        parts = dnbinom_parts(q, disp, lam)
        if parts is None:
            pv, a = mpf(1 if q == 0 else 0), mpf(0)
        else:
            pv, a = mpmath.exp(sum(parts)), sum(abs(v) for v in parts)
        c += pv
        w += pv * a / 2
        psum.append((1 - c) / 2)
        weight.append(w)
    return psum, weight


def lavec(opts, lam, lam_right, disp):
    """start_lavec of the restatement (start.r:28-44) with the weight W of every row."""
    m = opts.m
    if opts.termini != "both":
        psum, w = side(lam, disp, m)
        return (psum, w) if opts.termini == "5p" else (psum[::-1], w[::-1])
    half = m // 2
    psum, w = side(lam, disp, half)
    right, w_right = (psum, w) if opts.same_overhangs else side(lam_right, disp, half)
    return psum + right[::-1], w + w_right[::-1]


def lnfact_constant(counts):
    """function.r:124-128."""
    total = mpf(0)
    for row in counts:
        for lin in range(4):
            total += mpmath.loggamma(_mp(row[lin].sum()) + 1) - sum(mpmath.loggamma(_mp(v) + 1) for v in row[lin])
    return total


def loglik(table, nu, acgt, opts, x):
    """(log-likelihood, sum |term|, sum_i |dl/dla_i| W_i) of a parameter vector inside its ranges, every count's probability
    positive (logLikFunOneBaseFast, function.r:113-136; logLikAll, function.r:142-161)."""
    with mp.workdps(DIGITS):
        counts = M.counts(table)
        x, nu, acgt = [_mp(v) for v in x], [_mp(v) for v in nu], [_mp(v) for v in acgt]
        rho = mpf(1) if opts.fix_ti_tv else x[M.RHO]
        t = pmat(x[M.THETA], rho, acgt, opts.fix_ti_tv)
        la, weight = lavec(opts, x[M.LAMBDA], x[M.LAMBDAR], x[M.DISP])
        dd, ds = x[M.DELTAD], x[M.DELTAS]
        value, total, sens = lnfact_constant(counts), mpf(0), mpf(0)
        for i in range(opts.m):
            mix = la[i] * ds + dd * (1 - la[i])
            pct, pga = nu[i] * mix, (1 - nu[i]) * mix
            dct, dga = nu[i] * (ds - dd), (1 - nu[i]) * (ds - dd)           # d pct / d la, d pga / d la
            slope = mpf(0)
            for lin in range(4):
                p = (t[lin][0] + t[lin][2] * pga, t[lin][1] * (1 - pct), t[lin][2] * (1 - pga), t[lin][1] * pct + t[lin][3])
                dp = (t[lin][2] * dga, -t[lin][1] * dct, -t[lin][2] * dga, t[lin][1] * dct)
                for k in range(4):
                    term = _mp(counts[i, lin, k]) * mpmath.log(p[k])
                    value += term
                    total += abs(term)
                    slope += _mp(counts[i, lin, k]) * dp[k] / p[k]
            sens += abs(slope) * weight[i]
        return value, total, sens
