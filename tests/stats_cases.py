"""The cases the statistical stage's tests share: tables drawn from the model, and the chains of the parity tests with their
restatement (computed once per process)."""

import functools

import numpy as np

import stats_model as M

ACGT = (0.29, 0.21, 0.22, 0.28)
TRUTH = (0.012, 1.3, 0.02, 0.6, 0.35, 0.25, 1.6)        # Theta, Rho, DeltaD, DeltaS, Lambda, LambdaRight, LambdaDisp
PARITY_RUN = dict(n_rand=4, n_adjust=2, n_burn=150, n_iter=300)

# name: (m, termini, options of the chain, seed, chain id)
PARITY = {
    "full": (24, "both", dict(diff_hangs=True, var_disp=True), 11, 3),
    "m2": (2, "both", dict(diff_hangs=True, var_disp=True), 12, 0),
    "5p": (24, "5p", dict(var_disp=True), 13, 5),
}


def fixed_nu(m, termini):
    if termini == "both":
        return np.concatenate([np.ones(m // 2), np.zeros(m // 2)])
    return np.ones(m) if termini == "5p" else np.zeros(m)


@functools.lru_cache(maxsize=None)
def model_table(m, termini, per_row, seed, diff_hangs=True):
    """A table drawn from the model at TRUTH (HKY85, fixed nicks)."""
    opts = M.Options(m, termini, diff_hangs=diff_hangs and termini == "both", var_disp=True)
    table = M.simulate_table(np.random.default_rng(seed), opts, ACGT, fixed_nu(m, termini), TRUTH, per_row)
    table.setflags(write=False)
    return table


def parity_inputs(name):
    m, termini, flags, seed, chain_id = PARITY[name]
    return model_table(m, termini, 4000, 100 + seed), fixed_nu(m, termini), M.Options(m, termini, **flags), seed, chain_id


@functools.lru_cache(maxsize=None)
def parity_restatement(name):
    table, nu, opts, seed, chain_id = parity_inputs(name)
    chain = M.Chain(table, nu, ACGT, opts, seed, chain_id)
    trace = chain.run(**PARITY_RUN)
    trace.setflags(write=False)
    return chain, trace
