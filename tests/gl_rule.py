"""--pileup-likelihoods, restated by brute force as the issue words the rule (no line of csrc/mdx_pileup_key.h, none of
mapdamage_amd/pileup.py): every record's alignment expanded column by column (tests/pileup_rule.py), every pair that adds to a
base counter looked up in a table built here from the formulas, the sums and the ten values made in Python integers, the files
written from them.  The CPU tests hold the header's host build and the emitters to it, the GPU tests the device stage and the
command line's files.

GATK's model (ANGSD -GL 2): e = min(0.75, 10^(-q/10)); an observed base b has the term HOM = log(1 - e) under a genotype bb,
HET = log((1 - e)/2 + e/6) under a heterozygous one that holds b, NO = log(e/3) otherwise; a term is stored as
round(term * 2^24)."""

import math

import numpy as np

from tests import pileup_rule as PR

GENOTYPES = ("AA", "AC", "AG", "AT", "CC", "CG", "CT", "GG", "GT", "TT")
HOM, HET, NO = 0, 1, 2
SCALE = 1 << 24


def table():
    """[94][3] of Python integers."""
    out = []
    for q in range(94):
        e = min(0.75, 10 ** (-q / 10))
        out.append([round(math.ldexp(x, 24)) for x in (math.log(1 - e), math.log((1 - e) / 2 + e / 6), math.log(e / 3))])
    return out


TABLE = table()


def pair_qualities(record, sites_of_tid, k5=0, k3=0, min_qual=0, noqual=30):
    """{position: (counter 0 .. 7, quality 0 .. 93, the record has qualities)} of the sites at which the counted record adds."""
    flag, lib, tid, pos, cigar, seq, qual = record
    with_qual = PR.has_qualities(seq, qual)
    index = {at: q for at, q, op in PR.columns(pos, cigar) if at is not None and q is not None}
    out = {}
    for p, cls in PR.site_classes(record, sites_of_tid, k5, k3, min_qual).items():
        if cls < 8:
            out[p] = (cls, min(int(qual[index[p]]), 93) if with_qual else noqual, with_qual)
    return out


def brute(records, n_libraries, lengths, sites, k5=0, k3=0, min_qual=0, noqual=30):
    """-> (sums: a list per site of 24 Python integers, [strand][base][HOM HET NO]; dict of the pairs added and those of them
    from records without qualities)."""
    index = {site: g for g, site in enumerate(sites)}
    by_tid = {}
    for t, p in sites:
        by_tid.setdefault(t, set()).add(p)
    sums = [[0] * 24 for _ in sites]
    counts = dict(added=0, without_qualities=0)
    for record in records:
        flag, lib, tid, pos, cigar = record[:5]
        if PR.classify(flag, lib, tid, pos, cigar, n_libraries, lengths) != PR.COUNTED:
            continue
        for p, (cls, q, with_qual) in pair_qualities(record, by_tid.get(tid, set()), k5, k3, min_qual, noqual).items():
            row = sums[index[(tid, p)]]
            for term in range(3):
                row[3 * cls + term] += TABLE[q][term]
            counts["added"] += 1
            counts["without_qualities"] += 0 if with_qual else 1
    return sums, counts


def strands(alleles, single_strand):
    """(the + strand is eligible, the - strand is)"""
    if alleles is not None and single_strand:
        if set(alleles) == {"C", "T"}:
            return False, True
        if set(alleles) == {"G", "A"}:
            return True, False
    return True, True


def likelihoods(row, counters, alleles=None, single_strand=False):
    """The ten values (Python integers, the best one 0), the index of the best and Bases of one site from its 24 sums and its
    counters.  ``alleles``: (ref, alt) as letters, or None."""
    eligible = [s for s, ok in enumerate(strands(alleles, single_strand)) if ok]
    bases = sum(int(counters[4 * s + b]) for s in eligible for b in range(4))
    if bases == 0:
        return [0] * 10, 0, 0
    S = [[sum(int(row[(4 * s + b) * 3 + term]) for s in eligible) for term in range(3)] for b in range(4)]
    logl = []
    for a1 in range(4):
        for a2 in range(a1, 4):
            logl.append(sum(S[b][HOM] if a1 == a2 == b else S[b][HET] if a1 != a2 and b in (a1, a2) else S[b][NO] for b in range(4)))
    top = max(logl)
    return [v - top for v in logl], logl.index(top), bases


def all_likelihoods(sums, counters, alleles=None, single_strand=False):
    """-> (gl [sites][10] int64, best [sites], bases [sites])"""
    out = [likelihoods(sums[g], counters[g], None if alleles is None else alleles[g], single_strand) for g in range(len(sums))]
    return np.array([o[0] for o in out], np.int64).reshape(-1, 10), [o[1] for o in out], [o[2] for o in out]


# ---------------------------------------------------------------------- the files
def likelihoods_text(names, sites, ids, alleles, gl, best, bases):
    rows = ["\t".join(["Sequence", "Position", "Id", "Ref", "Alt", "Bases"] + list(GENOTYPES) + ["Best"])]
    for g, (t, p) in enumerate(sites):
        ref, alt = alleles[g] if alleles is not None else (".", ".")
        row = [names[t], str(p + 1), ids[g] if ids is not None else ".", ref, alt, str(int(bases[g]))]
        row += ["%.6f" % (int(v) / SCALE / math.log(10)) for v in gl[g]]
        rows.append("\t".join(row + [GENOTYPES[int(best[g])] if bases[g] else "."]))
    return "\n".join(rows) + "\n"


def summary_text(path, min_qual, k5, k3, single_strand, noqual, bases, counts):
    head = ["SitesFile", "MinBaseQual", "MaskEnds", "SingleStrandMode", "NoQualQuality", "Sites", "SitesWithBases", "BaseObservations", "WithoutQualities"]
    row = [str(path), str(min_qual), "%d,%d" % (k5, k3), str(int(single_strand)), str(noqual), str(len(bases)), str(sum(1 for n in bases if n >= 1)),
           str(counts["added"]), str(counts["without_qualities"])]
    return "\t".join(head) + "\n" + "\t".join(row) + "\n"


def beagle_text(names, sites, alleles, gl, bases):
    rows = ["marker\tallele1\tallele2\tInd0\tInd0\tInd0"]
    for g, (t, p) in enumerate(sites):
        ref, alt = (PR.BASES.index(a) for a in alleles[g])
        if bases[g]:
            three = [math.exp(int(gl[g][GENOTYPES.index("".join(sorted(PR.BASES[x] + PR.BASES[y], key=PR.BASES.index)))]) / SCALE)
                     for x, y in ((ref, ref), (ref, alt), (alt, alt))]
            three = [x / sum(three) for x in three]
        else:
            three = [1 / 3] * 3
        rows.append("%s_%d\t%d\t%d\t%s" % (names[t], p + 1, ref, alt, "\t".join("%.6f" % x for x in three)))
    return "\n".join(rows) + "\n"


def log_line(noqual, bases, counts):
    return ("Pileup likelihoods: %d sites, %d with bases, %d base observations (%d from records without qualities, taken at %d)"
            % (len(bases), sum(1 for n in bases if n >= 1), counts["added"], counts["without_qualities"], noqual))


LIKELIHOOD_FLOATS, BEAGLE_FLOATS = range(6, 16), range(3, 6)      # the columns of either file that hold reals


def same_text(got, want, float_columns, tolerance=1.01e-6):
    """Two files of the same layout: integers and letters exact, every real of the rows behind the header within ``tolerance`` —
    both sides print six decimals of reals that agree to about 1e-12, so they differ by one unit of the last place at the most."""
    a, b = got.split("\n"), want.split("\n")
    assert len(a) == len(b), (len(a), len(b))
    assert a[0] == b[0]
    for number, (x, y) in enumerate(zip(a[1:], b[1:]), 2):
        fx, fy = x.split("\t"), y.split("\t")
        assert len(fx) == len(fy), (number, x, y)
        for column, (u, v) in enumerate(zip(fx, fy)):
            if column in float_columns:
                assert len(u.split(".")[1]) == 6 and abs(float(u) - float(v)) <= tolerance, (number, x, y)
            else:
                assert u == v, (number, x, y)
    return True
