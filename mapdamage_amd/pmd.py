"""The post-mortem damage score (PMDS; Skoglund et al. 2014, PNAS 111:2229, "PMDtools") of ``--by-pmd-score``: the table of
its terms, the thresholds in the score's fixed point, the names of the groups and the text of ``by_pmd/``.  The rule itself —
which columns of a record add which term — is ``csrc/mdx_pmd_key.h`` (include/mdx.h ``mdx_set_strata_pmd``); everything
here is host arithmetic in Python doubles, so that the table is the same bytes wherever it is built."""

import io
import math

import numpy as np

N_Z = 256               # distances the table knows: a base further from its end takes the last one's term
N_QCOLS = 95            # quality columns: 0 .. 93 and column 94, eps = 0 (a record without qualities)
N_BINS = 82             # bins of the score histogram: half units over [-20, 20) and one bin beyond either end
FX_BITS = 24            # the score's fixed point: 2^24 to the unit
DEFAULT_MODEL = (0.3, 0.01, 0.001)
MAX_THRESHOLDS = 15


def check_model(p, C, pi):
    """``--pmd-model p,C,pi``: 0 < p < 1, 0 <= C, p + C < 1, 0 < pi < 1 (every D_z then lies in [C, p + C], inside (0, 1)
    but for C = 0 far from the end, and no logarithm below meets 0)."""
    p, C, pi = float(p), float(C), float(pi)
    if not (0.0 < p < 1.0 and 0.0 <= C and p + C < 1.0 and 0.0 < pi < 1.0):
        raise ValueError("PMD model p,C,pi = %g,%g,%g: needs 0 < p < 1, 0 <= C, p + C < 1 and 0 < pi < 1" % (p, C, pi))
    return p, C, pi


def term_table(p=DEFAULT_MODEL[0], C=DEFAULT_MODEL[1], pi=DEFAULT_MODEL[2]):
    """int32 [2][256][95]: ``[0]`` the term of a match, ``[1]`` of a mismatch, at distance ``z = 1 .. 256`` from the end, for
    quality column ``q``, ``round(ldexp(term, 24))``:

        D_z = p (1-p)^(z-1) + C                     eps_q = 10^(-q/10) / 3 (q = 0 .. 93), eps_94 = 0
        Pm(D) = (1-D)(1-eps)(1-pi) + D eps (1-pi) + eps pi (1-D)
        match = log(Pm(D_z) / Pm(0))                mismatch = log((1 - Pm(D_z)) / (1 - Pm(0)))

    in Python doubles and in exactly this order of operations."""
    p, C, pi = check_model(p, C, pi)
    out = np.zeros((2, N_Z, N_QCOLS), np.int32)
    for q in range(N_QCOLS):
        eps = 10 ** (-q / 10) / 3 if q < N_QCOLS - 1 else 0.0

        def pm(D):
            return (1 - D) * (1 - eps) * (1 - pi) + D * eps * (1 - pi) + eps * pi * (1 - D)
        pm0 = pm(0.0)
        for z in range(1, N_Z + 1):
            D = p * (1 - p) ** (z - 1) + C
            pmd = pm(D)
            out[0, z - 1, q] = round(math.ldexp(math.log(pmd / pm0), FX_BITS))
            out[1, z - 1, q] = round(math.ldexp(math.log((1 - pmd) / (1 - pm0)), FX_BITS))
    return out


def threshold_fx(t):
    """A threshold in the score's fixed point: the least integer S with S 2^-24 >= t, ``ceil(t 2^24)``."""
    return int(math.ceil(math.ldexp(float(t), FX_BITS)))


def check_thresholds(thresholds):
    """1 to 15 strictly increasing thresholds, as floats."""
    ts = [float(t) for t in thresholds]
    if not 1 <= len(ts) <= MAX_THRESHOLDS:
        raise ValueError("PMD thresholds: %d given, 1 to %d are possible" % (len(ts), MAX_THRESHOLDS))
    if any(not math.isfinite(t) or abs(t) >= 2.0 ** 38 for t in ts):
        # (their fixed point is an int64; no score comes near: 2^31 bases of the largest term are below 2^34)
        raise ValueError("PMD thresholds must be finite numbers below 2^38 in size")
    if any(b <= a for a, b in zip(ts, ts[1:])):
        raise ValueError("PMD thresholds must be strictly increasing (sorted, none twice): %s" % ",".join("%g" % t for t in ts))
    if len(set(threshold_fx(t) for t in ts)) != len(ts):
        raise ValueError("PMD thresholds closer than the score's resolution of 2^-24: %s" % ",".join("%g" % t for t in ts))
    return ts


def group_names(thresholds):
    """``<t1``, ``[t1,t2)``, ..., ``>=tk``, numbers as ``%g``."""
    ts = ["%g" % t for t in thresholds]
    return ["<" + ts[0]] + ["[%s,%s)" % (a, b) for a, b in zip(ts, ts[1:])] + [">=" + ts[-1]]


def groups_text(names, kept):
    """``by_pmd/groups.tsv``: index, group, kept reads (``kept[g]``)."""
    out = io.StringIO()
    out.write("Index\tGroup\tReads\n")
    for g, name in enumerate(names):
        out.write("%d\t%s\t%d\n" % (g, name, int(kept[g])))
    return out.getvalue()


def bin_edges(b):
    """(low, high) of histogram bin ``b`` as text: half units from -20, the first and last bin open-ended."""
    low = "-inf" if b == 0 else "%g" % (-20 + (b - 1) / 2)
    high = "inf" if b == N_BINS - 1 else "%g" % (-20 + b / 2)
    return low, high


def scores_text(libraries, hist):
    """``by_pmd/scores.tsv``: ``Sample Library Low High Reads`` — every library (the emitters' order: sorted by sample and
    library) and all 82 bins; ``hist[library][bin]`` in the order of ``libraries``."""
    hist = np.asarray(hist).reshape(len(libraries), N_BINS)
    out = io.StringIO()
    out.write("Sample\tLibrary\tLow\tHigh\tReads\n")
    for (sample, library), li in sorted((tuple(lib), i) for i, lib in enumerate(libraries)):
        for b in range(N_BINS):
            low, high = bin_edges(b)
            out.write("%s\t%s\t%s\t%s\t%d\n" % (sample, library, low, high, int(hist[li, b])))
    return out.getvalue()
