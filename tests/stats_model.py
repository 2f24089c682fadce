"""Host restatement of the statistical stage (numpy), written from the reference's R files — cited as file:line of
mapdamage/r/stats/ — and of the random-number scheme of include/mdx.h (mdx_stats_*).  The GPU tests compare the device
sampler with it; nothing here is used by the package."""

import math

import numpy as np

COLUMNS = ("A", "C", "G", "T", "A.C", "A.G", "A.T", "C.A", "C.G", "C.T", "G.A", "G.C", "G.T", "T.A", "T.C", "T.G")
THETA, RHO, DELTAD, DELTAS, LAMBDA, LAMBDAR, DISP, LOGLIK = range(8)
START = (-math.log((-(0.00396 / 3) + .25) * 4), 1.0, 0.0285, 0.269, 0.27, 0.27, 1.0)       # runGeneral.r:27-37, main.r:45
PROPOSAL_SD = (0.0003, 0.001, 0.001, 0.009, 0.008, 0.008, 0.015)                              # runGeneral.r:10-18
DISP_STARTS = (0.5, 1, 2, 3, 4, 50, 100, 150, 400)                                            # start.r:65
RHO_STARTS = (0.5, .75, 1, 1.25, 1.5)                                                         # start.r:66
_lgamma = np.vectorize(math.lgamma, otypes=[float])


# ---- Philox4x32-10 ----------------------------------------------------------------------------------------------------
def philox(seed, chain, c0, c1, c2, c3):
    """Four words per counter (arrays broadcast), key (seed, chain)."""
    c = [np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, int(chain) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xFFFFFFFF),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(0xFFFFFFFF)]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def uniforms(seed, chain, phase, it, update, draw):
    w = philox(seed, chain, phase, it, update, draw)
    def one(lo, hi):
        return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) + 0.5
    return one(w[0], w[1]) * 2.0 ** -53, one(w[2], w[3]) * 2.0 ** -53


def normal(seed, chain, phase, it, update, draw):
    u0, u1 = uniforms(seed, chain, phase, it, update, draw)
    return np.sqrt(-2.0 * np.log(u0)) * np.cos(6.283185307179586476925286766559 * u1)


def pick(u, n):
    return np.minimum((np.asarray(u) * n).astype(np.int64), n - 1)


# ---- the model ----------------------------------------------------------------------------------------------------------
def qmat_hky85(tmu, rho, acgt):
    """function.r:50-64."""
    acgt = np.asarray(acgt, float)
    q = np.array([[0, rho, 1, rho], [rho, 0, rho, 1], [1, rho, 0, rho], [rho, 1, rho, 0]], float) * acgt
    return tmu * (q - np.diag(q.sum(axis=1)))


def pmat(tmu, rho, acgt, jukes_cantor=False):
    """getPmat (function.r:8-64): exp(Q) through the eigen-decomposition of Q, rows = the base substituted.  (The
    reference's ``solve(t(B), E %*% t(B))`` is the transpose of this matrix; the two agree for Jukes–Cantor.)"""
    if jukes_cantor:
        return np.full((4, 4), 1 / 4 - math.exp(-tmu) / 4) + np.diag(np.full(4, math.exp(-tmu)))   # function.r:44-48
    values, vectors = np.linalg.eig(qmat_hky85(tmu, rho, acgt))
    return np.real(vectors @ np.diag(np.exp(values)) @ np.linalg.inv(vectors))


def dnbinom(x, size, prob):
    """R's dnbinom as seqProbVecLambda calls it (function.r:76).  prob == 1 and size == 0 are the point mass at 0; prob == 0
    (Lambda = 0, which the updates let through) puts no mass on any count, so the overhang stays at 1/2 in every row."""
    x = np.asarray(x, float)
    if prob == 1.0 or size == 0.0:
        return (x == 0).astype(float)
    log_prob = math.log(prob) if prob > 0.0 else -math.inf                  # (math.log raises at 0)
    return np.exp(_lgamma(x + size) - math.lgamma(size) - _lgamma(x + 1.0) + size * log_prob + x * math.log1p(-prob))


def seq_prob_vec(lam, disp, m, termini="both"):
    """seqProbVecLambda (function.r:74-88)."""
    psum = (1 - np.cumsum(dnbinom(np.arange(m), disp, lam))) / 2
    if termini == "both":
        return np.concatenate([psum[:m // 2], psum[:m // 2][::-1]])
    return psum if termini == "5p" else psum[::-1]


def counts(table):
    """[m][lin][k]: the S matrices of logLikAll (function.r:148-158) from an m x 16 table in COLUMNS order."""
    table = np.asarray(table, float)
    s = np.zeros((table.shape[0], 4, 4))
    for lin in range(4):
        sub = table[:, 4 + 3 * lin:7 + 3 * lin]
        others = [k for k in range(4) if k != lin]
        s[:, lin, others] = sub
        s[:, lin, lin] = table[:, lin] - ((sub[:, 0] + sub[:, 1]) + sub[:, 2])
    return s


def lnfact_constant(table):
    """Sum of lnfact(Gen) - sum lnfact(S) (function.r:124-128): the part of the likelihood no parameter moves."""
    s = counts(table)
    return math.fsum([math.lgamma(n + 1) for n in np.asarray(table)[:, :4].ravel()] + [-math.lgamma(v + 1) for v in s.ravel()])


def loglik_terms(table, theta_mat, deltad, deltas, la, nu):
    """The terms S * log(pDam) [m][lin][k] of logLikFunOneBaseFast (function.r:113-136)."""
    s = counts(table)
    la, nu = np.asarray(la, float)[:, None], np.asarray(nu, float)[:, None]
    mix = la * deltas + deltad * (1 - la)
    pct, pga = nu * mix, (1 - nu) * mix
    t = theta_mat[None, :, :]
    p = np.stack([t[:, :, 0] * 1 + t[:, :, 2] * pga, t[:, :, 1] * (1 - pct), t[:, :, 2] * (1 - pga),
                  t[:, :, 1] * pct + t[:, :, 3] * 1], axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s * np.log(p)


class Options:
    def __init__(self, m, termini="both", jukes_cantor=False, diff_hangs=False, var_disp=False):
        self.m, self.termini, self.fix_ti_tv, self.same_overhangs, self.fix_disp = m, termini, jukes_cantor, not diff_hangs, not var_disp


def start_lavec(opts, lam, lam_right, disp):
    """The overhang vector of logLikAllOptimize (start.r:28-44)."""
    la = seq_prob_vec(lam, disp, opts.m, opts.termini)
    if opts.termini == "both" and not opts.same_overhangs:
        la = np.concatenate([la[:opts.m // 2], seq_prob_vec(lam_right, disp, opts.m, "both")[opts.m // 2:]])
    return la


def loglik_of(table, const, nu, acgt, opts, x, with_abs=False):
    """The log-likelihood of a parameter vector as mdx_stats_loglik defines it: -inf outside the parameters' ranges."""
    rho = 1.0 if opts.fix_ti_tv else x[RHO]
    right = opts.termini == "both" and not opts.same_overhangs
    ok = (x[THETA] >= 0 and rho > 0 and 0 <= x[DELTAD] <= 1 and 0 <= x[DELTAS] <= 1 and 0 <= x[LAMBDA] <= 1
          and (not right or 0 <= x[LAMBDAR] <= 1) and x[DISP] >= 0)
    if not ok:
        return (-math.inf, 0.0) if with_abs else -math.inf
    terms = loglik_terms(table, pmat(x[THETA], rho, acgt, opts.fix_ti_tv), x[DELTAD], x[DELTAS],
                         start_lavec(opts, x[LAMBDA], x[LAMBDAR], x[DISP]), nu)
    value = const + float(terms.sum())
    return (value, float(np.abs(terms).sum())) if with_abs else value


def log_dnorm(x, mean, sd):
    z = (x - mean) / sd
    return -0.5 * z * z - math.log(sd) - 0.91893853320467274178


def prior(p, x):
    """priorPropose.r:4-52, inside the ranges the updates let through."""
    if p in (THETA, RHO):
        return log_dnorm(x, 1.0, 500.0)
    if p == DISP:
        return math.log(2) + log_dnorm(x, 0.0, 100.0)
    return 0.0


class Chain:
    """One chain: the start search, runGibbs (function.r:247-276) over the updates of postConditonal.r, adjustPropVar
    (function.r:225-245), driven by the Philox stream of (seed, chain id).  ``margin`` is the smallest
    |log u - (new - old)| any accept step has seen: how far the run is from a decision that rounding could flip."""

    def __init__(self, table, nu, acgt, opts, seed, chain_id):
        self.table, self.nu, self.acgt, self.o = np.asarray(table, float), np.asarray(nu, float), np.asarray(acgt, float), opts
        self.const = lnfact_constant(table)
        self.seed, self.chain_id = seed, chain_id
        self.par = list(START)
        self.sd = list(PROPOSAL_SD)
        self.margin = math.inf

    def lik(self, theta_mat, dd, ds, la):
        if dd < 0 or dd > 1 or ds < 0 or ds > 1:
            return -math.inf
        return self.const + float(loglik_terms(self.table, theta_mat, dd, ds, la, self.nu).sum())

    def search(self, n_rand):
        o, best = self.o, -math.inf
        for r in range(n_rand):
            u = np.concatenate([np.stack(uniforms(self.seed, self.chain_id, 0, r, 0, d)) for d in range(4)])
            x = [0.0] * 7
            x[THETA], x[DELTAD], x[DELTAS], x[LAMBDA] = u[0], u[1], u[2], u[3]
            x[LAMBDAR] = u[3] if o.same_overhangs else u[4]
            x[DISP] = 1.0 if o.fix_disp else DISP_STARTS[int(pick(u[5], 9))]
            x[RHO] = 1.0 if o.fix_ti_tv else RHO_STARTS[int(pick(u[6], 5))]
            ll = loglik_of(self.table, self.const, self.nu, self.acgt, o, x)
            if ll > best:
                best, self.par = ll, [float(v) for v in x]
                if o.same_overhangs:
                    self.par[LAMBDAR] = 0.27

    def begin(self):
        """main.r:73-90, 160-173."""
        o, p = self.o, self.par
        self.theta_mat = pmat(p[THETA], p[RHO], self.acgt, o.fix_ti_tv)
        self.la = seq_prob_vec(p[LAMBDA], p[DISP], o.m, o.termini)
        la0 = self.la
        if not o.same_overhangs:
            self.la_right = seq_prob_vec(p[LAMBDAR], p[DISP], o.m, o.termini)
            la0 = np.concatenate([self.la[:o.m // 2], self.la_right[o.m // 2:]])
        self.old_lik = self.lik(self.theta_mat, p[DELTAD], p[DELTAS], la0)

    def update(self, phase, it, p):
        o, par, half = self.o, self.par, self.o.m // 2
        star = par[p] + self.sd[p] * float(normal(self.seed, self.chain_id, phase, it, p, 0))
        if (p == THETA and star < 0) or (p == RHO and star <= 0) or (p == DISP and star < 0):
            return
        if p in (DELTAD, DELTAS, LAMBDA, LAMBDAR) and (star < 0 or star > 1):
            return
        mat, dd, ds, la = self.theta_mat, par[DELTAD], par[DELTAS], self.la
        if p == THETA:
            mat = pmat(star, par[RHO], self.acgt, o.fix_ti_tv)
        elif p == RHO:
            mat = pmat(par[THETA], star, self.acgt, o.fix_ti_tv)
        elif p == DELTAD:
            dd = star
        elif p == DELTAS:
            ds = star
        elif p == LAMBDA:                                                   # postConditonal.r:98-105
            la = seq_prob_vec(star, par[DISP], o.m, o.termini)
            if not o.same_overhangs:
                la = np.concatenate([la[:half], self.la_right[half:]])
        elif p == LAMBDAR:                                                  # :129-131
            la = np.concatenate([self.la[:half], seq_prob_vec(star, par[DISP], o.m, o.termini)[half:]])
        else:                                                               # :152-158
            la = seq_prob_vec(par[LAMBDA], star, o.m, o.termini)
            if not o.same_overhangs:
                la = np.concatenate([la[:half], seq_prob_vec(par[LAMBDAR], star, o.m, o.termini)[half:]])
        new_func = self.lik(mat, dd, ds, la)
        new_lik, old_lik = new_func + prior(p, star), self.old_lik + prior(p, par[p])
        log_u = math.log(float(uniforms(self.seed, self.chain_id, phase, it, p, 1)[0]))
        if not math.isnan(new_lik - old_lik):
            self.margin = min(self.margin, abs(log_u - (new_lik - old_lik)))
        if log_u < new_lik - old_lik:                                       # metroDesc (function.r:66-72)
            par[p], self.old_lik = star, new_func
            if p in (THETA, RHO):
                self.theta_mat = mat
            elif p == LAMBDAR:
                self.la_right = la                                          # :137 (cp$laVec stays as it is)
            elif p in (LAMBDA, DISP):
                self.la = la

    def gibbs(self, phase, n):
        o, out = self.o, np.zeros((n, 8))
        for it in range(n):
            self.update(phase, it, THETA)
            if not o.fix_ti_tv:
                self.update(phase, it, RHO)
            self.update(phase, it, DELTAD)
            self.update(phase, it, DELTAS)
            self.update(phase, it, LAMBDA)
            if not o.same_overhangs:
                self.update(phase, it, LAMBDAR)
            if not o.fix_disp:
                self.update(phase, it, DISP)
            out[it, :7] = self.par
            out[it, LOGLIK] = self.lik(self.theta_mat, self.par[DELTAD], self.par[DELTAS], self.la)     # function.r:270
        return out

    def adjust(self, out):
        """adjustPropVar (function.r:225-245); accRat counts distinct consecutive values."""
        o = self.o
        for p in range(7):
            if (p == LAMBDAR and o.same_overhangs) or (p == DISP and o.fix_disp) or (p == RHO and o.fix_ti_tv):
                continue
            rat = acc_rat(out[:, p])
            if rat < 0.1:
                self.sd[p] = self.sd[p] / 2
            elif rat > 0.3:
                self.sd[p] = self.sd[p] * 2

    def run(self, n_rand, n_adjust, n_burn, n_iter):
        self.search(n_rand)
        self.start = list(self.par)
        self.begin()
        rounds = max(n_adjust, 1)
        for r in range(rounds):                                             # main.r:176-192
            out = self.gibbs(1 + r, n_burn)
            if n_adjust > 0:
                self.adjust(out)
        return self.gibbs(1 + rounds, n_iter)                               # main.r:197


def acc_rat(column):
    column = np.asarray(column)
    return (1 + int(np.count_nonzero(column[1:] != column[:-1]))) / len(column)


def correcting(trace, nu, acgt, opts, seed, chain_id, phase, n_pred):
    """postPredCheck / simPredCheck (function.r:279-414): the means of damProb and damProbGA over n_pred draws, every
    parameter picked from its own column of the trace by the draws of ``phase``.  [m][2]."""
    trace, nu, m = np.asarray(trace), np.asarray(nu, float), opts.m
    s = np.arange(n_pred)
    u = np.stack([x for d in range(4) for x in uniforms(seed, chain_id, phase, s, 0, d)])            # [8][n_pred]
    cols = (LAMBDA, DISP, LAMBDAR, DISP, DELTAS, DELTAD, THETA, RHO)
    v = [trace[pick(u[d], len(trace)), cols[d]] for d in range(8)]
    ct, ga = np.zeros(m), np.zeros(m)
    for i in range(n_pred):
        if opts.same_overhangs:
            la = seq_prob_vec(v[0][i], v[1][i], m, opts.termini)
        else:                                                               # (function.r:291-297: termini left at "both")
            la = np.concatenate([seq_prob_vec(v[0][i], v[1][i], m)[:m // 2], seq_prob_vec(v[2][i], v[3][i], m)[m // 2:]])
        mat = pmat(v[6][i], v[7][i], acgt, opts.fix_ti_tv)
        mix = la * v[4][i] + v[5][i] * (1 - la)
        pct, pga = nu * mix, (1 - nu) * mix
        ct += mat[1, 1] * pct / (mat[1, 1] * pct + mat[1, 3])
        ga += mat[2, 2] * pga / (mat[2, 2] * pga + mat[2, 0])
    return np.stack([ct / n_pred, ga / n_pred], axis=1)


def simulate_table(rng, opts, acgt, nu, x, per_row):
    """A table drawn from the model at the parameter vector x: per_row bases of every reference base in every row."""
    mat = pmat(x[THETA], 1.0 if opts.fix_ti_tv else x[RHO], acgt, opts.fix_ti_tv)
    la = start_lavec(opts, x[LAMBDA], x[LAMBDAR], x[DISP])
    table = np.zeros((opts.m, 16))
    for i in range(opts.m):
        mix = la[i] * x[DELTAS] + x[DELTAD] * (1 - la[i])
        pct, pga = nu[i] * mix, (1 - nu[i]) * mix
        for lin in range(4):
            t = mat[lin]
            p = np.array([t[0] + t[2] * pga, t[1] * (1 - pct), t[2] * (1 - pga), t[1] * pct + t[3]])
            draw = rng.multinomial(per_row, p / p.sum())
            table[i, lin] = per_row
            table[i, 4 + 3 * lin:7 + 3 * lin] = [draw[k] for k in range(4) if k != lin]
    return table
