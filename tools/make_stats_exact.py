"""Generate tests/golden/stats_loglik_exact.npz: the log-likelihood of the statistical stage at the large dispersions of the
start search (start.r:65: 50, 100, 150, 400), evaluated with mpmath at 80 digits by tests/stats_exact.py.

    python tools/make_stats_exact.py

m in {24, 130, 256} x fixed / raw nick vector x 4 dispersions x 5 start-like vectors = 120 evaluations on tables of 10^6
bases a row (both termini, --diff-hangs, --var-disp, HKY85).  The fixture holds the inputs (tables, nick vectors, parameter
vectors) and, per evaluation, the exact value as a decimal string and rounded to double, sum |term| and the sensitivity
term of tests/stats_cases.py:exact_bound.  Needs mpmath; the tests that read the fixture do not."""

import pathlib
import sys

import mpmath
import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import stats_cases as C  # noqa: E402
import stats_exact as X  # noqa: E402
import stats_model as M  # noqa: E402

OUT = ROOT / "tests" / "golden" / "stats_loglik_exact.npz"
GROUPS = [(m, kind) for m in (24, 130, 256) for kind in ("fixed", "raw")]
LARGE_DISPS = M.DISP_STARTS[5:]
PER_CELL = 5


def main():
    rng = np.random.default_rng(4242)
    data = dict(acgt=np.array(C.ACGT), group_m=np.array([m for m, _ in GROUPS], np.int32),
                group_nu=np.array([kind for _, kind in GROUPS]))
    group_of, params, text, value, sum_abs, sens = [], [], [], [], [], []
    for g, (m, kind) in enumerate(GROUPS):
        seed = 700 + g
        table, nu = C.model_table(m, "both", 1_000_000, seed, nu_kind=kind), C.nu_of(kind, m, "both", seed)
        data["table_%d" % g], data["nu_%d" % g] = table.astype(np.int32), nu
        assert (data["table_%d" % g] == table).all()
        opts = M.Options(m, "both", diff_hangs=True, var_disp=True)
        for disp in LARGE_DISPS:
            for _ in range(PER_CELL):
                x = rng.uniform(size=7)
                x[M.DISP], x[M.RHO] = disp, rng.choice(M.RHO_STARTS)
                exact, total, s = X.loglik(table, nu, C.ACGT, opts, x)
                group_of.append(g), params.append(x), text.append(mpmath.nstr(exact, 50, strip_zeros=False))
                value.append(float(exact)), sum_abs.append(float(total)), sens.append(float(s))
                print("m %3d %-5s disp %3d  %s  sum|term| %.3g  sens %.3g" % (m, kind, disp, text[-1], total, s), flush=True)
    data.update(group_of=np.array(group_of, np.int32), params=np.array(params), exact_text=np.array(text), exact=np.array(value),
                sum_abs=np.array(sum_abs), sens=np.array(sens))
    np.savez_compressed(OUT, **data)
    print("%s: %d evaluations, %d bytes" % (OUT, len(value), OUT.stat().st_size))


if __name__ == "__main__":
    main()
