"""The Bayesian estimate of the damage parameters (mapdamage/r/stats/, driven by mapdamage/rscript.py:70-100) on the GPU.

The host's share: the ``m x 16`` data matrix of ``readMapDamData`` (data.r) from ``misincorporation.txt``, the base
frequencies of ``dnacomp_genome.csv`` (``readBaseFreqs``), the nick-frequency vector of main.r:98-148 and the three files
``writeMCMC`` (function.r:417-441) and main.r:225 write.  The chains themselves — start search, burn-in with the proposal
variances adjusted, the kept iterations, the correcting probabilities — run on the device, one wavefront per chain, any
number of chains (one per table set) in one launch: ``mdx_stats_run`` (include/mdx.h, csrc/mdx_stats.hip).

R lines are cited as file:line of mapdamage/r/stats/."""

import ctypes
import logging
import math
import pathlib

import numpy as np

NUCLEOTIDES = ("A", "C", "G", "T")
MISMATCHES = ("A.C", "A.G", "A.T", "C.A", "C.G", "C.T", "G.A", "G.C", "G.T", "T.A", "T.C", "T.G")      # data.r:3-7
COLUMNS = NUCLEOTIDES + MISMATCHES
PARAMETERS = ("Theta", "Rho", "DeltaD", "DeltaS", "Lambda", "LambdaRight", "LambdaDisp", "LogLik")      # function.r:251
TERMINI = {"both": 0, "5p": 1, "3p": 2}
MAX_ROWS = 256                                                                                           # MDX_STATS_MAX_M
N_PRED = 10000                                                                                           # function.r:355

ITER_CSV, SUMM_CSV, CORR_CSV = ("Stats_out_MCMC_iter.csv", "Stats_out_MCMC_iter_summ_stat.csv",
                                "Stats_out_MCMC_correct_prob.csv")


class StatsError(RuntimeError):
    pass


class StatsConfig(ctypes.Structure):
    """mdx_stats_config of include/mdx.h."""
    _fields_ = [(name, ctypes.c_int32) for name in ("m", "termini", "fix_ti_tv", "same_overhangs", "fix_disp", "n_rand",
                                                    "n_adjust", "n_burn", "n_iter", "n_pred")] + \
               [("seed", ctypes.c_uint32), ("reserved", ctypes.c_int32)]


class StatsOptions:
    """What the estimate takes from the command line (the environment of mapdamage/rscript.py:76-98)."""

    def __init__(self, seq_length=12, termini="both", rand=30, burn=10000, adjust=10, iterations=50000, var_disp=False,
                 jukes_cantor=False, diff_hangs=False, fix_nicks=False, use_raw_nick_freq=False, single_stranded=False,
                 seed=0, n_pred=N_PRED):
        self.seq_length, self.termini = int(seq_length), termini
        self.rand, self.burn, self.adjust, self.iterations = int(rand), int(burn), int(adjust), int(iterations)
        self.var_disp, self.jukes_cantor, self.diff_hangs = bool(var_disp), bool(jukes_cantor), bool(diff_hangs)
        self.fix_nicks, self.use_raw_nick_freq, self.single_stranded = bool(fix_nicks), bool(use_raw_nick_freq), bool(single_stranded)
        self.seed, self.n_pred = int(seed), int(n_pred)
        problem = self.problem()
        if problem:
            raise StatsError(problem)

    def problem(self):
        """Why these options cannot be run, or None."""
        if self.termini not in TERMINI:
            return "invalid termini %r" % (self.termini,)
        if self.fix_nicks + self.use_raw_nick_freq + self.single_stranded > 1:                          # config.py:477
            return "The options --use-raw-nick-freq, --fix-nicks and --single-stranded are mutually exclusive."
        if not (self.fix_nicks or self.use_raw_nick_freq or self.single_stranded):
            return ("the estimate needs one of --fix-nicks, --use-raw-nick-freq and --single-stranded: the reference's default "
                    "nick frequencies come from a smoothing spline of R's gam package, which this engine does not reproduce")
        if self.diff_hangs and self.termini != "both":                                                  # main.r:85-87
            return "Cannot use different overhangs with only the %s end" % self.termini
        if self.seq_length < 1 or self.rows > MAX_ROWS:
            return "--seq-length must be between 1 and %d" % (MAX_ROWS // 2 if self.termini == "both" else MAX_ROWS)
        if self.rand < 0 or self.adjust < 0 or self.burn < 1 or self.iterations < 1:
            return "--rand and --adjust must not be negative, --burn and --iter at least 1"
        if not 0 <= self.seed < 2 ** 32:
            return "--stats-seed must be between 0 and 2^32 - 1"
        return None

    @property
    def rows(self):
        return self.seq_length * (2 if self.termini == "both" else 1)

    @classmethod
    def from_args(cls, o):
        return cls(o.seq_length, o.termini, o.rand, o.burn, o.adjust, o.iter, o.var_disp, o.jukes_cantor, o.diff_hangs,
                   o.fix_nicks, o.use_raw_nick_freq, o.single_stranded, o.stats_seed)

    def config(self, m):
        return StatsConfig(m, TERMINI[self.termini], int(self.jukes_cantor), int(not self.diff_hangs), int(not self.var_disp),
                           self.rand, self.adjust, self.burn, self.iterations, self.n_pred, self.seed, 0)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def data_matrix(text, seq_length=12, termini="both"):
    """``readMapDamData`` (data.r:2-24) over the text of a ``misincorporation.txt``: the rows with ``Pos <= seq_length``, the
    positions of the 3p rows negated, one end alone for ``termini`` 5p / 3p, the 4 + 12 columns summed over samples,
    libraries and strands by position.  Returns (positions, matrix [m][16] in ``COLUMNS`` order; ``X.Y`` is the file's
    ``X>Y``).  Rows: 1 .. n, then -n .. -1 — the 5' positions first, each end read inwards and outwards as the vectors
    of main.r:81-110 are laid out (R's ``aggregate`` hands the groups back sorted, the negative positions first)."""
    if termini not in TERMINI:
        raise StatsError("invalid termini %r" % (termini,))
    lines = [line for line in text.splitlines() if line.strip() and not line.startswith("#")]
    if not lines:
        raise StatsError("misincorporation table is empty")
    header = lines[0].split("\t")
    at = {name: i for i, name in enumerate(header)}
    try:
        cols = [at[name.replace(".", ">")] for name in COLUMNS]
        end_at, pos_at = at["End"], at["Pos"]
    except KeyError as error:
        raise StatsError("misincorporation table lacks the column %s" % error)
    sums = {}
    for line in lines[1:]:
        fields = line.split("\t")
        pos, end = int(fields[pos_at]), fields[end_at]
        if pos > seq_length or (termini != "both" and end != termini):
            continue
        row = sums.setdefault(-pos if end == "3p" else pos, np.zeros(len(COLUMNS)))
        row += [int(fields[c]) for c in cols]
    positions = sorted(p for p in sums if p > 0) + sorted(p for p in sums if p < 0)
    if not positions:
        raise StatsError("misincorporation table holds no row for the requested termini and --seq-length")
    return positions, np.stack([sums[p] for p in positions])


def read_base_freqs(path):
    """``readBaseFreqs`` (data.r:27-32): A, C, G, T of ``dnacomp_genome.csv``; the checks of getPmat (function.r:10-13)."""
    from .composition import read_base_comp
    row = read_base_comp(path)
    acgt = [float(row[base]) for base in NUCLEOTIDES]
    check_base_freqs(acgt)
    return acgt


def check_base_freqs(acgt):
    if any(v >= 1 or v <= 0 for v in acgt):
        raise StatsError("The ACGT frequencies must be in the range 0 to 1")
    if abs(sum(acgt) - 1) > 1.5e-8:                                                                     # all.equal's tolerance
        raise StatsError("The ACGT frequencies do not sum to 1")


def nu_vector(table, termini="both", single_stranded=False, fix_nicks=False, use_raw_nick_freq=False):
    """The nick-frequency vector of main.r:98-148 for the three ways that need no ``gam``.  Returns (vector, warning or None)."""
    table = np.asarray(table, float)
    m = table.shape[0]
    constant = {"5p": np.ones(m), "3p": np.zeros(m)}.get(termini)
    if constant is None:
        constant = np.concatenate([np.ones(m // 2), np.zeros(m - m // 2)])
    if single_stranded:
        return np.ones(m), None                                                                        # main.r:98-100
    if fix_nicks:
        return constant, None                                                                          # :101-110
    if not use_raw_nick_freq:
        raise StatsError("the smoothed nick frequencies of the reference (gam) are not reproduced")
    col = {name: i for i, name in enumerate(COLUMNS)}
    with np.errstate(divide="ignore", invalid="ignore"):
        ct, ga = table[:, col["C.T"]] / table[:, col["C"]], table[:, col["G.A"]] / table[:, col["G"]]
        te = ct / (ga + ct)                                                                            # :114
    if np.isnan(te).any():                                                                             # :115-124
        return constant, "To few substitutions to assess the nick frequency, using constant nick frequency instead"
    return np.clip(te, 0.0, 1.0), None                                                                 # :128-145


def lnfact_constant(table):
    """The terms of logLikFunOneBaseFast (function.r:124-128) that no parameter moves, summed over rows and reference
    bases: ``lnfact(N) - sum lnfact(S)``."""
    table = np.asarray(table, float)
    terms = []
    for row in table:
        for lin in range(4):
            sub = row[4 + 3 * lin:7 + 3 * lin]
            same = row[lin] - ((sub[0] + sub[1]) + sub[2])
            terms += [math.lgamma(row[lin] + 1), -math.lgamma(same + 1)] + [-math.lgamma(v + 1) for v in sub]
    return math.fsum(terms)


# ---- the device ---------------------------------------------------------------------------------------------------------
def _library():
    from .engine import load_library
    lib = load_library()
    if not getattr(lib, "_stats_declared", False):
        p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        lib.mdx_stats_loglik.restype = lib.mdx_stats_run.restype = lib.mdx_stats_pmat.restype = ctypes.c_int
        lib.mdx_stats_loglik.argtypes = [i32, p, i32, p, p, p, p, i64, p, p, p]
        lib.mdx_stats_run.argtypes = [i32, p, i32, p, p, p, p, p, p, p, p, p, p]
        lib.mdx_stats_pmat.argtypes = [i32, i64, p, i32, p]
        lib._stats_declared = True
    return lib


def _ptr(array):
    return array.ctypes.data_as(ctypes.c_void_p)


def _check(lib, code, what):
    if code:
        from .engine import MdxError
        raise MdxError(code, "%s: %s" % (what, lib.mdx_strerror(code).decode()))


def _inputs(tables, nus, acgts, m):
    tables = np.ascontiguousarray(tables, dtype=np.float64).reshape(-1, m, 16)
    n = tables.shape[0]
    nus = np.ascontiguousarray(np.broadcast_to(np.asarray(nus, np.float64), (n, m)))
    acgts = np.ascontiguousarray(np.broadcast_to(np.asarray(acgts, np.float64), (n, 4)))
    if (tables < 0).any() or (nus < 0).any() or (nus > 1).any() or not np.isfinite(tables).all():
        raise StatsError("a table holds a negative or non-finite count, or a nick frequency outside [0, 1]")
    consts = np.array([lnfact_constant(t) for t in tables], np.float64)
    return tables, nus, acgts, consts


def loglik(tables, nus, acgts, table_of, params, options, device=0):
    """Log-likelihoods of parameter vectors (Theta, Rho, DeltaD, DeltaS, Lambda, LambdaRight, LambdaDisp), evaluation ``e`` on
    table ``table_of[e]``: ``mdx_stats_loglik``."""
    lib = _library()
    m = np.asarray(tables).shape[-2]
    tables, nus, acgts, consts = _inputs(tables, nus, acgts, m)
    params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 7)
    table_of = np.ascontiguousarray(table_of, dtype=np.int32)
    assert len(table_of) == len(params)
    out = np.zeros(len(params), np.float64)
    cfg = options.config(m)
    _check(lib, lib.mdx_stats_loglik(device, ctypes.byref(cfg), len(tables), _ptr(tables), _ptr(consts), _ptr(nus), _ptr(acgts),
                                     len(params), _ptr(table_of), _ptr(params), _ptr(out)), "mdx_stats_loglik")
    return out


def substitution_matrices(theta_rho_acgt, jukes_cantor=False, device=0):
    """[n][4][4] (row = the base substituted) for rows Theta, Rho, A, C, G, T: ``mdx_stats_pmat``."""
    lib = _library()
    x = np.ascontiguousarray(theta_rho_acgt, dtype=np.float64).reshape(-1, 6)
    out = np.zeros((len(x), 4, 4), np.float64)
    _check(lib, lib.mdx_stats_pmat(device, len(x), _ptr(x), int(bool(jukes_cantor)), _ptr(out)), "mdx_stats_pmat")
    return out


class Estimate:
    """One chain's outcome: ``trace`` [iterations][8] (``PARAMETERS``), ``prop_sd`` [7], ``acc`` [8], ``corr`` [m][2]
    (C.T, G.A), ``start`` [8]."""

    def __init__(self, trace, prop_sd, acc, corr, start):
        self.trace, self.prop_sd, self.acc, self.corr, self.start = trace, prop_sd, acc, corr, start


def run_chains(tables, nus, acgts, options, chain_ids=None, device=0):
    """One chain per table, all in one launch (``mdx_stats_run``).  ``chain_ids``: the second word of each chain's Philox
    key (default 0, 1, ...); a chain's outcome depends on its table, the options, the seed and that word alone."""
    lib = _library()
    m = np.asarray(tables).shape[-2]
    tables, nus, acgts, consts = _inputs(tables, nus, acgts, m)
    n = len(tables)
    ids = np.arange(n, dtype=np.uint32) if chain_ids is None else np.ascontiguousarray(chain_ids, dtype=np.uint32)
    assert len(ids) == n
    cfg = options.config(m)
    trace = np.zeros((n, options.iterations, 8), np.float64)
    prop_sd, acc = np.zeros((n, 7), np.float64), np.zeros((n, 8), np.float64)
    corr, start = np.zeros((n, m, 2), np.float64), np.zeros((n, 8), np.float64)
    _check(lib, lib.mdx_stats_run(device, ctypes.byref(cfg), n, _ptr(tables), _ptr(consts), _ptr(nus), _ptr(acgts), _ptr(ids),
                                  _ptr(trace), _ptr(prop_sd), _ptr(acc), _ptr(corr), _ptr(start)), "mdx_stats_run")
    return [Estimate(trace[k], prop_sd[k], acc[k], corr[k], start[k]) for k in range(n)]


# ---- outputs: the layout of R's write.csv -------------------------------------------------------------------------------------
def _num(value):
    """A number as write.csv prints it: 15 significant digits, ``NA`` / ``Inf`` spelled R's way."""
    value = float(value)
    if math.isnan(value):
        return "NA"
    if math.isinf(value):
        return "Inf" if value > 0 else "-Inf"
    return "%.15g" % value


def _write_csv(path, columns, names, rows):
    with open(path, "wt") as out:
        out.write(",".join('"%s"' % c for c in ("",) + tuple(columns)) + "\n")
        for name, row in zip(names, rows):
            out.write('"%s",' % name + ",".join(_num(v) for v in row) + "\n")


def quantile7(column, probs):
    """R's default (type 7) quantile: linear between the order statistics at h = (n - 1) p."""
    x = np.sort(np.asarray(column, float))
    h = (len(x) - 1) * np.asarray(probs, float)
    lo = np.floor(h).astype(int)
    hi = np.minimum(lo + 1, len(x) - 1)
    return x[lo] + (h - lo) * (x[hi] - x[lo])


def written_parameters(options):
    """The columns of writeMCMC (function.r:419-429), in its order."""
    names = ["Theta", "DeltaD", "DeltaS", "Lambda"]
    if not options.jukes_cantor:
        names.append("Rho")
    if options.diff_hangs:
        names.append("LambdaRight")
    if options.var_disp:
        names.append("LambdaDisp")
    return names + ["LogLik"]


def write_estimate(folder, estimate, positions, options):
    """``Stats_out_MCMC_iter.csv``, ``..._iter_summ_stat.csv`` (writeMCMC, function.r:417-441) and
    ``Stats_out_MCMC_correct_prob.csv`` (main.r:225, function.r:411-412)."""
    folder = pathlib.Path(folder)
    names = written_parameters(options)
    cols = [PARAMETERS.index(name) for name in names]
    out = estimate.trace[:, cols]
    n = len(out)
    _write_csv(folder / ITER_CSV, names, range(1, n + 1), out)
    probs = np.arange(41) * 0.025
    summary = [out.mean(axis=0), out.std(axis=0, ddof=1) if n > 1 else np.full(len(cols), np.nan), estimate.acc[cols]]
    quantiles = np.stack([quantile7(out[:, j], probs) for j in range(len(cols))], axis=1)
    labels = ["Mean", "Std.", "Acceptance ratio"] + ["%s%%" % ("%.7g" % (100 * p)) for p in probs]
    _write_csv(folder / SUMM_CSV, names, labels, list(summary) + list(quantiles))
    _write_csv(folder / CORR_CSV, ("Position", "C.T", "G.A"), range(1, len(positions) + 1),
               [(p, c, g) for p, (c, g) in zip(positions, estimate.corr)])


# ---- the stage ------------------------------------------------------------------------------------------------------------
def estimate_folders(folders, acgt, options, chain_ids=None, device=0, logger=None):
    """The estimate of every folder that holds a ``misincorporation.txt``, all chains in one launch; each folder gets its
    three files.  ``acgt``: the base frequencies (ignored with --jukes-cantor, main.r:33-39).  Returns the ``Estimate``s."""
    logger = logger or logging.getLogger(__name__)
    tables, nus, positions = [], [], []
    for folder in folders:
        pos, table = data_matrix((pathlib.Path(folder) / "misincorporation.txt").read_text(), options.seq_length, options.termini)
        if len(pos) != options.rows:
            raise StatsError("%s: the table holds %d of the %d positions the estimate needs (--seq-length %d beyond --length?)"
                             % (folder, len(pos), options.rows, options.seq_length))
        nu, warning = nu_vector(table, options.termini, options.single_stranded, options.fix_nicks, options.use_raw_nick_freq)
        if warning:
            logger.warning("%s", warning)
        tables.append(table), nus.append(nu), positions.append(pos)
    if not tables:
        return []
    acgt = [0.25] * 4 if options.jukes_cantor else list(acgt)
    logger.info("Performing Bayesian estimates: %d chain%s on the device (%d x %d burn-in, %d iterations, seed %d)",
                len(tables), "" if len(tables) == 1 else "s", max(options.adjust, 1), options.burn, options.iterations, options.seed)
    results = run_chains(np.stack(tables), np.stack(nus), acgt, options, chain_ids, device)
    for folder, pos, result in zip(folders, positions, results):
        write_estimate(folder, result, pos, options)
    return results
