// mdx_stats.hip — the Bayesian estimate of the damage parameters (mapdamage/r/stats/) on the device.
//
// One wavefront per chain, one block per wavefront; a launch holds any number of chains and runs a chain from its start
// search to its correcting probabilities.  The 4 x m x 4 terms S * log(pDam) of the likelihood are spread over the 64
// lanes: term t = 16 i + 4 lin + k (row i, reference base lin, read base k) belongs to lane t % 64, so a lane keeps one
// (lin, k) for good and walks the rows i = lane / 16 + 4 r.  A lane sums its terms in row order, the wave sums the lanes
// with a butterfly of fixed order: the value depends on the chain alone, never on what else is in the launch.  Everything
// is double.  The control flow of a chain is wave-uniform (every lane holds the chain's scalars and takes every decision
// from the same broadcast sum), which is what the block barriers around the LDS vectors need.
//
// Reference lines are cited as file:line of mapdamage/r/stats/.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mdx.h"

// (no fused multiply-adds: the host restatement of the model the tests compare with rounds every product)
#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr double kInf = __builtin_huge_val();

enum { P_THETA = 0, P_RHO, P_DELTAD, P_DELTAS, P_LAMBDA, P_LAMBDAR, P_DISP, P_LOGLIK, N_COL };

// ---- Philox4x32-10: key (seed, chain id), counter (phase, iteration, update index, draw index) ------------------------
struct Rng {
    uint32_t seed, chain;
};

__device__ inline void philox(const Rng &g, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]) {
    uint32_t k0 = g.seed, k1 = g.chain;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ inline double to_uniform(uint32_t lo, uint32_t hi) {
    const uint64_t x = ((uint64_t)hi << 32) | lo;
    return ((double)(x >> 11) + 0.5) * 0x1p-53;
}

// the two uniforms of one counter value
__device__ inline void uniforms(const Rng &g, uint32_t phase, uint32_t iter, uint32_t update, uint32_t draw, double &u0, double &u1) {
    uint32_t w[4];
    philox(g, phase, iter, update, draw, w);
    u0 = to_uniform(w[0], w[1]);
    u1 = to_uniform(w[2], w[3]);
}

__device__ inline double normal(const Rng &g, uint32_t phase, uint32_t iter, uint32_t update, uint32_t draw) {
    double u0, u1;
    uniforms(g, phase, iter, update, draw, u0, u1);
    return sqrt(-2.0 * log(u0)) * cos(kTwoPi * u1);          // Box–Muller
}

// ---- the substitution matrix, one entry (getPmat, function.r:8-64) ------------------------------------------------------
// Jukes–Cantor as jukesCantorPmat2 writes it (function.r:44-48).  HKY85 for the Q of qmatHKY85 (function.r:50-64: rate
// tmu pi_j for the transitions A<->G and C<->T, tmu rho pi_j for the transversions, rows summing to zero, not normalised)
// in closed form instead of eigen(): with s = sum pi, Pi = pi_j + pi_partner(j), e1 = exp(-tmu rho s) and
// e2 = exp(-tmu (Pi + rho (s - Pi))),
//   P[j][j]          = (pi_j + pi_j (s / Pi - 1) e1 + (Pi - pi_j) s / Pi e2) / s
//   P[partner(j)][j] = (pi_j + pi_j (s / Pi - 1) e1 - pi_j s / Pi e2) / s
//   P[other][j]      =  pi_j (1 - e1) / s
__device__ inline double pmat_entry(double tmu, double rho, const double *acgt, int jc, int i, int j) {
    if (jc) {
        const double e = exp(-tmu), off = 1.0 / 4 - e / 4;
        return i == j ? off + e : off;
    }
    const double s = ((acgt[0] + acgt[1]) + acgt[2]) + acgt[3];
    const double pj = acgt[j], big = pj + acgt[j ^ 2];
    const double e1 = exp(-(tmu * rho * s));
    if (((i ^ j) & 1) != 0) return pj * (1.0 - e1) / s;
    const double e2 = exp(-(tmu * (big + rho * (s - big))));
    const double base = pj + pj * (s / big - 1.0) * e1;
    return i == j ? (base + (big - pj) * s / big * e2) / s : (base - pj * s / big * e2) / s;
}

// ---- dnbinom(x, size, prob) through lgamma (seqProbVecLambda, function.r:76) ------------------------------------------------
// prob == 1 and size == 0 are the point mass at 0, as R's dnbinom has them (the logarithms alone would give NaN there).
__device__ inline double dnbinom(int x, double size, double prob) {
    if (prob == 1.0 || size == 0.0) return x == 0 ? 1.0 : 0.0;
    return exp(lgamma(x + size) - lgamma(size) - lgamma(x + 1.0) + size * log(prob) + x * log1p(-prob));
}

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v += __shfl_xor(v, d, kWave);
    return __shfl(v, 0, kWave);
}

// What a chain keeps in the LDS: the count of every term, the nick vector, the three overhang vectors, two scratch rows.
struct Lds {
    double *S, *nu, *la, *la_right, *la_star, *tmp, *pv, *acgt;
    __device__ Lds(double *base, int m)
        : S(base), nu(base + 16 * m), la(nu + m), la_right(la + m), la_star(la_right + m), tmp(la_star + m), pv(tmp + m), acgt(pv + m) {}
};
__host__ __device__ constexpr size_t lds_doubles(int m) { return (size_t)22 * m + 4; }

struct Model {
    int m, termini, fix_ti_tv, same_overhangs, fix_disp;
    double lnfact;
};

// seqProbVecLambda (function.r:74-88) into dst[0, m); ends with a barrier
__device__ void seq_prob(const Model &md, const Lds &l, double lambda, double disp, int termini, double *dst) {
    const int lane = threadIdx.x, n = termini == 0 ? md.m / 2 : md.m;
    for (int j = lane; j < n; j += kWave) l.pv[j] = dnbinom(j, disp, lambda);
    __syncthreads();
    for (int j = lane; j < n; j += kWave) {
        double c = 0;
        for (int q = 0; q <= j; ++q) c += l.pv[q];           // cumsum, in its order
        const double psum = (1.0 - c) / 2;
        if (termini != 2) dst[j] = psum;
        if (termini != 1) dst[md.m - 1 - j] = psum;
    }
    __syncthreads();
}

__device__ inline void copy_row(double *dst, const double *src, int from, int to) {
    for (int j = from + (int)threadIdx.x; j < to; j += kWave) dst[j] = src[j];
}

// The two matrix entries a lane's terms need (logLikFunOneBaseFast, function.r:119-122).
struct Coef { double c1, c2; };
__device__ inline Coef lane_coef(const Model &md, const Lds &l, double theta, double rho) {
    const int lin = (threadIdx.x >> 2) & 3, k = threadIdx.x & 3;
    const int a = k == 0 ? 0 : (k == 2 ? 2 : 1), b = k == 0 ? 2 : 3;
    Coef c;
    c.c1 = pmat_entry(theta, rho, l.acgt, md.fix_ti_tv, lin, a);
    c.c2 = pmat_entry(theta, rho, l.acgt, md.fix_ti_tv, lin, b);
    return c;
}

// logLikAll (function.r:142-161); la is an LDS row that a barrier has made visible
__device__ double loglik(const Model &md, const Lds &l, Coef cf, double deltad, double deltas, const double *la) {
    if (deltad < 0 || deltad > 1 || deltas < 0 || deltas > 1) return -kInf;
    const int lane = threadIdx.x, k = lane & 3;
    double acc = 0;
    for (int i = lane >> 4; i < md.m; i += 4) {
        const double lam = la[i], nu = l.nu[i];
        const double mix = lam * deltas + deltad * (1 - lam);
        const double pct = nu * mix, pga = (1 - nu) * mix;
        double p;
        if (k == 0) p = cf.c1 * 1 + cf.c2 * pga;
        else if (k == 1) p = cf.c1 * (1 - pct);
        else if (k == 2) p = cf.c1 * (1 - pga);
        else p = cf.c1 * pct + cf.c2 * 1;
        acc += l.S[16 * i + (lane & 15)] * log(p);
    }
    return md.lnfact + wave_sum(acc);
}

__device__ inline double log_dnorm(double x, double mean, double sd) {
    const double z = (x - mean) / sd;
    return -0.5 * z * z - log(sd) - 0.91893853320467274178;     // log(sqrt(2 pi))
}

// priorPropose.r:4-52 for the values the updates let through (inside their ranges: dbeta(x, 1, 1, log) is 0)
__device__ inline double prior(int p, double x) {
    if (p == P_THETA || p == P_RHO) return log_dnorm(x, 1.0, 500.0);
    if (p == P_DISP) return 0.69314718055994530942 + log_dnorm(x, 0.0, 100.0);
    return 0.0;
}

struct Chain {
    double par[7];      // Theta, Rho, DeltaD, DeltaS, Lambda, LambdaRight, LambdaDisp
    double old_lik;
    Coef cf;            // of (Theta, Rho): cp$ThetaMat
};

// the overhang vector of logLikAllOptimize (start.r:28-44), into la_star
__device__ void start_lavec(const Model &md, const Lds &l, double lambda, double lambda_right, double disp) {
    seq_prob(md, l, lambda, disp, md.termini, l.la_star);
    if (md.termini == 0 && !md.same_overhangs) {
        seq_prob(md, l, lambda_right, disp, 0, l.tmp);
        copy_row(l.la_star, l.tmp, md.m / 2, md.m);
        __syncthreads();
    }
}

// log-likelihood of a whole parameter vector, as the start search and mdx_stats_loglik see it: -inf outside the
// parameters' ranges (the bounds of start.r:13 and of the updates' early returns), logLikAll inside
__device__ double loglik_of(const Model &md, const Lds &l, const double *x) {
    const double rho = md.fix_ti_tv ? 1.0 : x[P_RHO], disp = x[P_DISP];
    const bool right = md.termini == 0 && !md.same_overhangs;
    const bool bad = !(x[P_THETA] >= 0) || !(rho > 0) || !(x[P_DELTAD] >= 0 && x[P_DELTAD] <= 1) || !(x[P_DELTAS] >= 0 && x[P_DELTAS] <= 1) ||
                     !(x[P_LAMBDA] >= 0 && x[P_LAMBDA] <= 1) || (right && !(x[P_LAMBDAR] >= 0 && x[P_LAMBDAR] <= 1)) || !(disp >= 0);
    if (bad) return -kInf;
    start_lavec(md, l, x[P_LAMBDA], x[P_LAMBDAR], disp);
    return loglik(md, l, lane_coef(md, l, x[P_THETA], rho), x[P_DELTAD], x[P_DELTAS], l.la_star);
}

// One Metropolis update (postConditonal.r).  An out-of-range proposal returns having consumed its normal and no uniform.
template <int p>
__device__ void update(const Model &md, const Lds &l, const Rng &g, Chain &c, const double (&sd)[7], uint32_t phase, uint32_t it) {
    const double star = c.par[p] + sd[p] * normal(g, phase, it, p, 0);
    if (p == P_THETA) { if (star < 0) return; }
    else if (p == P_RHO) { if (star <= 0) return; }
    else if (p == P_DISP) { if (star < 0) return; }
    else if (star < 0 || star > 1) return;

    const int half = md.m / 2;
    Coef cf = c.cf;
    double dd = c.par[P_DELTAD], ds = c.par[P_DELTAS];
    const double *la = l.la;
    if (p == P_THETA) cf = lane_coef(md, l, star, c.par[P_RHO]);
    else if (p == P_RHO) cf = lane_coef(md, l, c.par[P_THETA], star);
    else if (p == P_DELTAD) dd = star;
    else if (p == P_DELTAS) ds = star;
    else {
        la = l.la_star;
        if (p == P_LAMBDA) {                                            // postConditonal.r:98-105
            seq_prob(md, l, star, c.par[P_DISP], md.termini, l.la_star);
            if (!md.same_overhangs) { copy_row(l.la_star, l.la_right, half, md.m); __syncthreads(); }
        } else if (p == P_LAMBDAR) {                                    // :129-131
            seq_prob(md, l, star, c.par[P_DISP], md.termini, l.la_star);
            copy_row(l.la_star, l.la, 0, half);
            __syncthreads();
        } else {                                                        // :152-158
            seq_prob(md, l, c.par[P_LAMBDA], star, md.termini, l.la_star);
            if (!md.same_overhangs) {
                seq_prob(md, l, c.par[P_LAMBDAR], star, md.termini, l.tmp);
                copy_row(l.la_star, l.tmp, half, md.m);
                __syncthreads();
            }
        }
    }
    const double new_func = loglik(md, l, cf, dd, ds, la);
    const double new_lik = new_func + prior(p, star), old_lik = c.old_lik + prior(p, c.par[p]);
    double u0, u1;
    uniforms(g, phase, it, p, 1, u0, u1);
    if (log(u0) < new_lik - old_lik) {                                  // metroDesc (function.r:66-72); NaN rejects
        c.par[p] = star;
        c.old_lik = new_func;
        if (p == P_THETA || p == P_RHO) c.cf = cf;
        else if (p == P_LAMBDAR) { copy_row(l.la_right, l.la_star, 0, md.m); __syncthreads(); }     // :137 (cp$laVec stays)
        else if (p == P_LAMBDA || p == P_DISP) { copy_row(l.la, l.la_star, 0, md.m); __syncthreads(); }
    }
}

struct RunArgs {
    mdx_stats_config cfg;
    const double *tables, *lnfact, *nu, *acgt;
    const uint32_t *chain_id;
    double *trace, *prop_sd, *acc, *corr, *start;
};

// the m x 16 table of data.r (A C G T A.C A.G A.T C.A C.G C.T G.A G.C G.T T.A T.C T.G) as the 4 x 4 counts of every row
// (function.r:148-158), the nick vector and the base frequencies, into the LDS
__device__ void load_chain(const Lds &l, int m, const double *table, const double *nu, const double *acgt) {
    for (int t = threadIdx.x; t < 16 * m; t += kWave) {
        const double *row = table + (size_t)(t >> 4) * 16;
        const int lin = (t >> 2) & 3, k = t & 3;
        const double *sub = row + 4 + 3 * lin;
        l.S[t] = k == lin ? row[lin] - ((sub[0] + sub[1]) + sub[2]) : sub[k - (k > lin)];
    }
    for (int j = threadIdx.x; j < m; j += kWave) l.nu[j] = nu[j];
    if (threadIdx.x < 4) l.acgt[threadIdx.x] = acgt[threadIdx.x];
    __syncthreads();
}

// runGibbs (function.r:247-276): n iterations of the seven updates; the trace is kept when `trace` is given, the distinct
// consecutive values of every column are counted (accRat, function.r:220-223)
__device__ void run_phase(const Model &md, const Lds &l, const Rng &g, Chain &c, const double (&sd)[7], uint32_t phase, int n, double *trace,
                          int (&distinct)[N_COL]) {
    double prev[N_COL];
#pragma unroll
    for (int q = 0; q < N_COL; ++q) { distinct[q] = 0; prev[q] = 0; }
    for (int it = 0; it < n; ++it) {
        update<P_THETA>(md, l, g, c, sd, phase, it);
        if (!md.fix_ti_tv) update<P_RHO>(md, l, g, c, sd, phase, it);
        update<P_DELTAD>(md, l, g, c, sd, phase, it);
        update<P_DELTAS>(md, l, g, c, sd, phase, it);
        update<P_LAMBDA>(md, l, g, c, sd, phase, it);
        if (!md.same_overhangs) update<P_LAMBDAR>(md, l, g, c, sd, phase, it);
        if (!md.fix_disp) update<P_DISP>(md, l, g, c, sd, phase, it);
        // function.r:270 evaluates the likelihood again, with cp$laVec.  With the same overhangs those are the arguments
        // old_lik was computed from, so it is that value; with --diff-hangs cp$laVec can lag behind (postConditonal.r:137)
        const double ll = md.same_overhangs ? c.old_lik : loglik(md, l, c.cf, c.par[P_DELTAD], c.par[P_DELTAS], l.la);
#pragma unroll
        for (int q = 0; q < N_COL; ++q) {
            const double v = q == P_LOGLIK ? ll : c.par[q < 7 ? q : 0];
            if (it == 0 || v != prev[q]) ++distinct[q];
            prev[q] = v;
            if (trace && threadIdx.x == 0) trace[(size_t)it * N_COL + q] = v;
        }
    }
}

__device__ inline int pick(double u, int n) {
    const int i = (int)(u * n);
    return i < n ? i : n - 1;
}

__global__ __launch_bounds__(kWave) void k_stats_run(RunArgs a) {
    extern __shared__ double lds_base[];
    const mdx_stats_config &cfg = a.cfg;
    const int chain = blockIdx.x, m = cfg.m;
    const Lds l(lds_base, m);
    const Model md{m, cfg.termini, cfg.fix_ti_tv, cfg.same_overhangs, cfg.fix_disp, a.lnfact[chain]};
    const Rng g{cfg.seed, a.chain_id[chain]};
    load_chain(l, m, a.tables + (size_t)chain * m * 16, a.nu + (size_t)chain * m, a.acgt + (size_t)chain * 4);

    // start values (runGeneral.r:27-37, main.r:45-51) and initial proposal SDs (runGeneral.r:10-18)
    Chain c;
    c.par[P_THETA] = -log((-(0.00396 / 3) + .25) * 4);
    c.par[P_RHO] = 1; c.par[P_DELTAD] = 0.0285; c.par[P_DELTAS] = 0.269;
    c.par[P_LAMBDA] = 0.27; c.par[P_LAMBDAR] = 0.27; c.par[P_DISP] = 1;
    double sd[7] = {0.0003, 0.001, 0.001, 0.009, 0.008, 0.008, 0.015};

    // the --rand starts of start.r:60-66, each evaluated where Nelder–Mead would begin; the best one is the start
    double best = -kInf;
    for (int r = 0; r < cfg.n_rand; ++r) {
        double x[7], u[8];
#pragma unroll
        for (int d = 0; d < 4; ++d) uniforms(g, 0, r, 0, d, u[2 * d], u[2 * d + 1]);
        const double disps[9] = {0.5, 1, 2, 3, 4, 50, 100, 150, 400}, rhos[5] = {0.5, .75, 1, 1.25, 1.5};
        x[P_THETA] = u[0]; x[P_DELTAD] = u[1]; x[P_DELTAS] = u[2]; x[P_LAMBDA] = u[3];
        x[P_LAMBDAR] = md.same_overhangs ? u[3] : u[4];
        x[P_DISP] = md.fix_disp ? 1.0 : disps[pick(u[5], 9)];
        x[P_RHO] = md.fix_ti_tv ? 1.0 : rhos[pick(u[6], 5)];
        const double ll = loglik_of(md, l, x);
        if (ll > best) {
            best = ll;
            for (int q = 0; q < 7; ++q) c.par[q] = x[q];
            if (md.same_overhangs) c.par[P_LAMBDAR] = 0.27;          // (start.r:95-97: only asked-for parameters move)
        }
    }

    // main.r:73-90, 160-173
    c.cf = lane_coef(md, l, c.par[P_THETA], c.par[P_RHO]);
    seq_prob(md, l, c.par[P_LAMBDA], c.par[P_DISP], md.termini, l.la);
    if (!md.same_overhangs) {
        seq_prob(md, l, c.par[P_LAMBDAR], c.par[P_DISP], md.termini, l.la_right);
        copy_row(l.la_star, l.la, 0, m / 2);
        copy_row(l.la_star, l.la_right, m / 2, m);
        __syncthreads();
        c.old_lik = loglik(md, l, c.cf, c.par[P_DELTAD], c.par[P_DELTAS], l.la_star);
    } else {
        c.old_lik = loglik(md, l, c.cf, c.par[P_DELTAD], c.par[P_DELTAS], l.la);
    }
    if (a.start && threadIdx.x == 0) {
        for (int q = 0; q < 7; ++q) a.start[(size_t)chain * N_COL + q] = c.par[q];
        a.start[(size_t)chain * N_COL + P_LOGLIK] = c.old_lik;
    }

    // main.r:176-192: the burn-in rounds with adjustPropVar (function.r:225-245) after each, or one plain burn-in
    int distinct[N_COL];
    const int rounds = cfg.n_adjust > 0 ? cfg.n_adjust : 1;
    for (int r = 0; r < rounds; ++r) {
        run_phase(md, l, g, c, sd, 1 + r, cfg.n_burn, nullptr, distinct);
        if (cfg.n_adjust > 0)
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                if ((q == P_LAMBDAR && md.same_overhangs) || (q == P_DISP && md.fix_disp) || (q == P_RHO && md.fix_ti_tv)) continue;
                const double rat = (double)distinct[q] / cfg.n_burn;
                if (rat < 0.1) sd[q] = sd[q] / 2;
                else if (rat > 0.3) sd[q] = sd[q] * 2;
            }
    }
    double *trace = a.trace + (size_t)chain * cfg.n_iter * N_COL;
    run_phase(md, l, g, c, sd, 1 + rounds, cfg.n_iter, trace, distinct);     // main.r:197
    if (threadIdx.x == 0) {
        for (int q = 0; q < 7; ++q) a.prop_sd[(size_t)chain * 7 + q] = sd[q];
        for (int q = 0; q < N_COL; ++q) a.acc[(size_t)chain * N_COL + q] = (double)distinct[q] / cfg.n_iter;
    }
    // the trace (lane 0's stores) is read back by every lane below
    __threadfence();
    __syncthreads();

    // postPredCheck / simPredCheck (function.r:279-414): damProb and damProbGA averaged over n_pred draws, every
    // parameter drawn from its own column of the trace
    double sum_ct[4] = {0, 0, 0, 0}, sum_ga[4] = {0, 0, 0, 0};            // rows lane, lane + 64, ... (m <= 256)
    const uint32_t pred_phase = 2 + rounds;
    for (int s = 0; s < cfg.n_pred; ++s) {
        double u[8];
#pragma unroll
        for (int d = 0; d < 4; ++d) uniforms(g, pred_phase, s, 0, d, u[2 * d], u[2 * d + 1]);
        // draws 0..7: Lambda, LambdaDisp, LambdaRight, LambdaDisp (again, for the right side), DeltaS, DeltaD, Theta, Rho
        const int cols[8] = {P_LAMBDA, P_DISP, P_LAMBDAR, P_DISP, P_DELTAS, P_DELTAD, P_THETA, P_RHO};
        double v[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) v[d] = trace[(size_t)pick(u[d], cfg.n_iter) * N_COL + cols[d]];
        if (md.same_overhangs) {
            seq_prob(md, l, v[0], v[1], md.termini, l.la_star);
        } else {                                                            // (function.r:291-297: termini left at "both")
            seq_prob(md, l, v[0], v[1], 0, l.la_star);
            seq_prob(md, l, v[2], v[3], 0, l.tmp);
            copy_row(l.la_star, l.tmp, m / 2, m);
            __syncthreads();
        }
        const double cc = pmat_entry(v[6], v[7], l.acgt, md.fix_ti_tv, 1, 1), ct = pmat_entry(v[6], v[7], l.acgt, md.fix_ti_tv, 1, 3);
        const double gg = pmat_entry(v[6], v[7], l.acgt, md.fix_ti_tv, 2, 2), ga = pmat_entry(v[6], v[7], l.acgt, md.fix_ti_tv, 2, 0);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int i = threadIdx.x + kWave * n;
            if (i >= m) break;
            const double lam = l.la_star[i], nu = l.nu[i];
            const double mix = lam * v[4] + v[5] * (1 - lam);
            const double pct = nu * mix, pga = (1 - nu) * mix;
            sum_ct[n] += cc * pct / (cc * pct + ct);
            sum_ga[n] += gg * pga / (gg * pga + ga);
        }
        __syncthreads();                                                    // la_star is rewritten by the next draw
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int i = threadIdx.x + kWave * n;
        if (i >= m) break;
        a.corr[((size_t)chain * m + i) * 2] = sum_ct[n] / cfg.n_pred;
        a.corr[((size_t)chain * m + i) * 2 + 1] = sum_ga[n] / cfg.n_pred;
    }
}

struct LoglikArgs {
    mdx_stats_config cfg;
    const double *tables, *lnfact, *nu, *acgt, *params;
    const int32_t *table_of;
    double *out;
};

__global__ __launch_bounds__(kWave) void k_stats_loglik(LoglikArgs a) {
    extern __shared__ double lds_base[];
    const int m = a.cfg.m, t = a.table_of[blockIdx.x];
    const Lds l(lds_base, m);
    const Model md{m, a.cfg.termini, a.cfg.fix_ti_tv, a.cfg.same_overhangs, a.cfg.fix_disp, a.lnfact[t]};
    load_chain(l, m, a.tables + (size_t)t * m * 16, a.nu + (size_t)t * m, a.acgt + (size_t)t * 4);
    const double ll = loglik_of(md, l, a.params + (size_t)blockIdx.x * 7);
    if (threadIdx.x == 0) a.out[blockIdx.x] = ll;
}

__global__ void k_stats_pmat(int64_t n, const double *in, int jc, double *out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 16) return;
    const double *x = in + (t >> 4) * 6;
    out[t] = pmat_entry(x[0], x[1], x + 2, jc, (int)(t >> 2) & 3, (int)t & 3);
}

// device buffers of one call, released on every way out
struct Buffers {
    std::vector<void *> all;
    ~Buffers() { for (void *p : all) (void)hipFree(p); }
    template <typename T> hipError_t put(T *&dev, const T *host, size_t count) {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, count ? count * sizeof(T) : sizeof(T));
        if (e != hipSuccess) return e;
        all.push_back(p);
        dev = (T *)p;
        return host && count ? hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    }
};

bool config_ok(const mdx_stats_config *c) {
    if (!c || c->m < 1 || c->m > MDX_STATS_MAX_M || c->termini < 0 || c->termini > 2) return false;
    if (c->termini == 0 && (c->m & 1)) return false;
    if (!c->same_overhangs && c->termini != 0) return false;                // main.r:85-87
    return true;
}

#define STATS_TRY(call)                   \
    do {                                  \
        if ((call) != hipSuccess) {       \
            (void)hipGetLastError();      \
            return MDX_ERR_HIP;           \
        }                                 \
    } while (0)

}  // namespace

extern "C" int mdx_stats_pmat(int32_t device, int64_t n, const double *theta_rho_acgt, int32_t jukes_cantor, double *out) {
    if (n < 0 || n > (1 << 24) || (n && (!theta_rho_acgt || !out))) return MDX_ERR_ARG;
    if (!n) return MDX_OK;
    STATS_TRY(hipSetDevice(device));
    Buffers b;
    double *d_in = nullptr, *d_out = nullptr;
    STATS_TRY(b.put(d_in, theta_rho_acgt, (size_t)n * 6));
    STATS_TRY(b.put(d_out, (const double *)nullptr, (size_t)n * 16));
    k_stats_pmat<<<dim3((unsigned)((n * 16 + 255) / 256)), dim3(256), 0, 0>>>(n, d_in, jukes_cantor, d_out);
    STATS_TRY(hipGetLastError());
    STATS_TRY(hipMemcpy(out, d_out, (size_t)n * 16 * sizeof(double), hipMemcpyDeviceToHost));
    return MDX_OK;
}

extern "C" int mdx_stats_loglik(int32_t device, const mdx_stats_config *cfg, int32_t n_tables, const double *tables, const double *lnfact,
                                const double *nu, const double *acgt, int64_t n, const int32_t *table_of, const double *params, double *loglik) {
    if (!config_ok(cfg) || n_tables < 1 || n < 0 || n > (1 << 24) || !tables || !lnfact || !nu || !acgt) return MDX_ERR_ARG;
    if (!n) return MDX_OK;
    if (!table_of || !params || !loglik) return MDX_ERR_ARG;
    for (int64_t i = 0; i < n; ++i)
        if (table_of[i] < 0 || table_of[i] >= n_tables) return MDX_ERR_ARG;
    STATS_TRY(hipSetDevice(device));
    Buffers b;
    LoglikArgs a{};
    a.cfg = *cfg;
    const size_t m = (size_t)cfg->m;
    double *d_tables, *d_lnfact, *d_nu, *d_acgt, *d_params, *d_out;
    int32_t *d_of;
    STATS_TRY(b.put(d_tables, tables, n_tables * m * 16));
    STATS_TRY(b.put(d_lnfact, lnfact, (size_t)n_tables));
    STATS_TRY(b.put(d_nu, nu, n_tables * m));
    STATS_TRY(b.put(d_acgt, acgt, (size_t)n_tables * 4));
    STATS_TRY(b.put(d_params, params, (size_t)n * 7));
    STATS_TRY(b.put(d_of, table_of, (size_t)n));
    STATS_TRY(b.put(d_out, (const double *)nullptr, (size_t)n));
    a.tables = d_tables; a.lnfact = d_lnfact; a.nu = d_nu; a.acgt = d_acgt; a.params = d_params; a.table_of = d_of; a.out = d_out;
    k_stats_loglik<<<dim3((unsigned)n), dim3(kWave), lds_doubles(cfg->m) * sizeof(double), 0>>>(a);
    STATS_TRY(hipGetLastError());
    STATS_TRY(hipMemcpy(loglik, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return MDX_OK;
}

extern "C" int mdx_stats_run(int32_t device, const mdx_stats_config *cfg, int32_t n_chains, const double *tables, const double *lnfact,
                             const double *nu, const double *acgt, const uint32_t *chain_id, double *trace, double *prop_sd, double *acc,
                             double *corr, double *start) {
    if (!config_ok(cfg) || n_chains < 0 || n_chains > (1 << 20)) return MDX_ERR_ARG;
    if (cfg->n_rand < 0 || cfg->n_adjust < 0 || cfg->n_burn < 1 || cfg->n_iter < 1 || cfg->n_pred < 1) return MDX_ERR_ARG;
    if (!n_chains) return MDX_OK;
    if (!tables || !lnfact || !nu || !acgt || !chain_id || !trace || !prop_sd || !acc || !corr) return MDX_ERR_ARG;
    STATS_TRY(hipSetDevice(device));
    Buffers b;
    RunArgs a{};
    a.cfg = *cfg;
    const size_t m = (size_t)cfg->m, nc = (size_t)n_chains, n_trace = nc * (size_t)cfg->n_iter * N_COL;
    double *d_tables, *d_lnfact, *d_nu, *d_acgt, *d_trace, *d_sd, *d_acc, *d_corr, *d_start;
    uint32_t *d_id;
    STATS_TRY(b.put(d_tables, tables, nc * m * 16));
    STATS_TRY(b.put(d_lnfact, lnfact, nc));
    STATS_TRY(b.put(d_nu, nu, nc * m));
    STATS_TRY(b.put(d_acgt, acgt, nc * 4));
    STATS_TRY(b.put(d_id, chain_id, nc));
    STATS_TRY(b.put(d_trace, (const double *)nullptr, n_trace));
    STATS_TRY(b.put(d_sd, (const double *)nullptr, nc * 7));
    STATS_TRY(b.put(d_acc, (const double *)nullptr, nc * N_COL));
    STATS_TRY(b.put(d_corr, (const double *)nullptr, nc * m * 2));
    STATS_TRY(b.put(d_start, (const double *)nullptr, nc * N_COL));
    a.tables = d_tables; a.lnfact = d_lnfact; a.nu = d_nu; a.acgt = d_acgt; a.chain_id = d_id;
    a.trace = d_trace; a.prop_sd = d_sd; a.acc = d_acc; a.corr = d_corr; a.start = d_start;
    k_stats_run<<<dim3((unsigned)n_chains), dim3(kWave), lds_doubles(cfg->m) * sizeof(double), 0>>>(a);
    STATS_TRY(hipGetLastError());
    STATS_TRY(hipDeviceSynchronize());
    STATS_TRY(hipMemcpy(trace, d_trace, n_trace * sizeof(double), hipMemcpyDeviceToHost));
    STATS_TRY(hipMemcpy(prop_sd, d_sd, nc * 7 * sizeof(double), hipMemcpyDeviceToHost));
    STATS_TRY(hipMemcpy(acc, d_acc, nc * N_COL * sizeof(double), hipMemcpyDeviceToHost));
    STATS_TRY(hipMemcpy(corr, d_corr, nc * m * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (start) STATS_TRY(hipMemcpy(start, d_start, nc * N_COL * sizeof(double), hipMemcpyDeviceToHost));
    return MDX_OK;
}
