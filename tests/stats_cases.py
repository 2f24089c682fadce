"""The cases the statistical stage's tests share: tables drawn from the model, and the chains of the parity tests with their
restatement (computed once per process)."""

import functools

import numpy as np

import stats_model as M

ACGT = (0.29, 0.21, 0.22, 0.28)
TRUTH = (0.012, 1.3, 0.02, 0.6, 0.35, 0.25, 1.6)        # Theta, Rho, DeltaD, DeltaS, Lambda, LambdaRight, LambdaDisp
PARITY_RUN = dict(n_rand=4, n_adjust=2, n_burn=150, n_iter=300)
PLAIN_RUN = dict(n_rand=0, n_adjust=0, n_burn=100, n_iter=200)      # the published start values, one burn-in, SDs untouched
HANGS_DISP = dict(diff_hangs=True, var_disp=True)

# name: (m, termini, options of the chain, seed, chain id, kind of nick vector, run)
PARITY = {
    "full": (24, "both", HANGS_DISP, 11, 3, "fixed", PARITY_RUN),
    "m2": (2, "both", HANGS_DISP, 12, 0, "fixed", PARITY_RUN),
    "5p": (24, "5p", dict(var_disp=True), 13, 5, "fixed", PARITY_RUN),
    # beyond the wave's 64 lanes, and row counts that leave the four 16-lane groups of the likelihood uneven
    "both256": (256, "both", HANGS_DISP, 21, 1, "fixed", PARITY_RUN),
    "both130raw": (130, "both", HANGS_DISP, 22, 2, "raw", PARITY_RUN),
    "5p67": (67, "5p", dict(var_disp=True), 23, 8, "raw", PARITY_RUN),
    "3p65": (65, "3p", dict(var_disp=True), 24, 4, "fixed", PARITY_RUN),
    "3p256": (256, "3p", dict(), 25, 5, "fixed", PARITY_RUN),
    # the model the command line runs by default, and its neighbours
    "default24": (24, "both", dict(), 26, 6, "fixed", PARITY_RUN),
    "jc24": (24, "both", dict(jukes_cantor=True), 27, 7, "fixed", PARITY_RUN),
    "ss24": (24, "both", dict(), 28, 8, "ones", PARITY_RUN),
    "plain24": (24, "both", HANGS_DISP, 31, 9, "fixed", PLAIN_RUN),
}
BEYOND_THE_WAVE = tuple(name for name, case in PARITY.items() if case[0] > 64)


def fixed_nu(m, termini):
    if termini == "both":
        return np.concatenate([np.ones(m // 2), np.zeros(m // 2)])
    return np.ones(m) if termini == "5p" else np.zeros(m)


def raw_nu(m, termini, rng):
    """What --use-raw-nick-freq gives: every entry strictly inside (0, 1), near the fixed vector."""
    return fixed_nu(m, termini) * 0.9 + rng.uniform(0.0, 0.1, m)


@functools.lru_cache(maxsize=None)
def nu_of(kind, m, termini, seed=0):
    """The nick vector of a kind: ``fixed``, ``raw`` (drawn from ``seed``) or ``ones`` (--single-stranded)."""
    nu = {"fixed": lambda: fixed_nu(m, termini), "raw": lambda: raw_nu(m, termini, np.random.default_rng(5000 + seed)),
          "ones": lambda: np.ones(m)}[kind]()
    nu.setflags(write=False)
    return nu


@functools.lru_cache(maxsize=None)
def model_table(m, termini, per_row, seed, diff_hangs=True, nu_kind="fixed"):
    """A table drawn from the model at TRUTH (HKY85) under the nick vector ``nu_of(nu_kind, m, termini, seed)``."""
    opts = M.Options(m, termini, diff_hangs=diff_hangs and termini == "both", var_disp=True)
    table = M.simulate_table(np.random.default_rng(seed), opts, ACGT, nu_of(nu_kind, m, termini, seed), TRUTH, per_row)
    table.setflags(write=False)
    return table


def parity_inputs(name):
    m, termini, flags, seed, chain_id, nu_kind, _ = PARITY[name]
    return (model_table(m, termini, 4000, 100 + seed, nu_kind=nu_kind), nu_of(nu_kind, m, termini, 100 + seed),
            M.Options(m, termini, **flags), seed, chain_id)


def parity_run(name):
    return PARITY[name][6]


@functools.lru_cache(maxsize=None)
def parity_restatement(name):
    table, nu, opts, seed, chain_id = parity_inputs(name)
    chain = M.Chain(table, nu, ACGT, opts, seed, chain_id)
    trace = chain.run(**parity_run(name))
    trace.setflags(write=False)
    return chain, trace


def loglik_gap(trace):
    """The smallest relative step of the LogLik column between consecutive rows whose parameters differ.  The acceptance
    ratio of that column counts its distinct consecutive values (accRat, function.r:220-223), so a step of the order of
    the rounding — a dispersion near 100 moves the overhangs of a short table by less than one ulp — lets two correct
    implementations count differently."""
    trace = np.asarray(trace)
    changed = (trace[1:, :7] != trace[:-1, :7]).any(axis=1)
    step = np.abs(trace[1:, 7] - trace[:-1, 7]) / np.abs(trace[1:, 7])
    return float(step[changed].min()) if changed.any() else np.inf


# ---- the bounds of the log-likelihood tests -----------------------------------------------------------------------------
U = 2.0 ** -53
C_LG = 4        # ulps allowed to one lgamma / log / log1p; see exact_bound


def side_rows(m, termini):
    """The rows one call of seqProbVecLambda fills: the depth of its cumsum."""
    return m // 2 if termini == "both" else m


def loglik_ops(m, termini):
    """The roundings on the way from the parameters to one sum of terms: the lane's summation (ceil(m / 4) rows and the six
    steps of the butterfly), the cumsum of seq_prob (one addition a row of its side) and the library calls behind a term
    (three lgamma at 4 ulp, log, log1p, exp and the term's own log at 1: 16)."""
    return -(-m // 4) + 6 + side_rows(m, termini) + 16


def loglik_k(m, termini):
    """K of the bound K 2^-53 sum |term| between the device and the restatement.  At m = 24 it is the 512 the test has always
    used, for every termini; beyond, the same allowance per rounding: 512 ops(m) / ops(24), rounded up.  (both: 922 at 66,
    1536 at 130, 2740 at 256; one end: 1024 at 65, 1034 at 66, 1822 at 130, 3368 at 256.)"""
    return -(-512 * loglik_ops(m, termini) // loglik_ops(24, termini))


def exact_bound(m, termini, sum_abs, sens):
    """How far a double evaluation may lie from the exact log-likelihood: U (K(m) sum |term| + C_LG sens).  ``sens`` is
    sum_i |dl / dla_i| sum_{q <= i} pv[q] A_q / 2 (tests/stats_exact.py:side): with a large dispersion the summands of
    log dnbinom reach the thousands, an error of C_LG ulp in each moves pv[q] by C_LG U A_q pv[q], the overhang la_i by
    half the running sum of those, and the likelihood by the slope dl / dla_i.  C_LG: the ROCm device library's ulp
    figures were not at hand, so it is measured on the host libm against mpmath over the arguments the fixture uses
    (q + size and q + 1 for q < 128, size in 50 .. 400): lgamma at most 3.3 ulp, log, log1p and exp below 0.8; taken as 4."""
    return U * (loglik_k(m, termini) * sum_abs + C_LG * sens)


@functools.lru_cache(maxsize=None)
def exact_fixture():
    """tests/golden/stats_loglik_exact.npz (tools/make_stats_exact.py) as a dictionary; the tables as doubles."""
    import pathlib
    with np.load(pathlib.Path(__file__).resolve().parent / "golden" / "stats_loglik_exact.npz") as z:
        data = {key: z[key] for key in z.files}
    for key in data:
        if key.startswith("table_"):
            data[key] = data[key].astype(np.float64)
    return data
