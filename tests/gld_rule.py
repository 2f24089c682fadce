"""--pileup-damage-profile, restated by brute force as the issue words the rule (no line of csrc/mdx_pileup_key.h, none of
mapdamage_amd/pileup.py): the profile read and pooled in plain Python, the probabilities of the four true alleles written out as
the issue's table of the error model has them, a genotype's term as log(P(b|a1)/2 + P(b|a2)/2) — not the channel form —, every
pair that adds (tests/gl_rule.py, tests/pileup_rule.py) given its two distances in query bases, and the sums, the ten values and
the files made in Python integers.  The CPU tests hold the header's host build, the table and the emitters to it, the GPU tests
the device stage and the command line's files."""

import math

import numpy as np

from tests import gl_rule as GR
from tests import pileup_rule as PR

GENOTYPES = GR.GENOTYPES
PAIRS = [(a1, a2) for a1 in range(4) for a2 in range(a1, 4)]        # AA AC AG AT CC CG CT GG GT TT
A, C, G, T = range(4)


# ---------------------------------------------------------------------- the profile
def profile(text, k=20):
    """-> (d5, d3): per end the K + 1 rows (substitutions, bases, rate), the last the tail.  Raises ValueError."""
    lines = [line for line in text.split("\n") if line.strip() and not line.startswith("#")]
    if not lines:
        raise ValueError("no header")
    head = lines[0].split("\t")
    at = {name: head.index(name) for name in ("End", "Pos", "C", "G", "C>T", "G>A")}        # (ValueError: a missing column)
    cells = {"5p": {}, "3p": {}}
    for line in lines[1:]:
        f = line.split("\t")
        if len(f) <= max(at.values()):
            raise ValueError("a short line")
        end = f[at["End"]]
        if end not in cells:
            raise ValueError("End")
        for name in ("Pos", "C", "G", "C>T", "G>A"):
            if not (f[at[name]].isascii() and f[at[name]].isdigit()):
                raise ValueError(name)
        z, c, g, ct, ga = (int(f[at[name]]) for name in ("Pos", "C", "G", "C>T", "G>A"))
        if ct > c or ga > g or z < 1:
            raise ValueError("counts")
        sub, base = (ct, c) if end == "5p" else (ga, g)
        was = cells[end].get(z, (0, 0))
        cells[end][z] = (was[0] + sub, was[1] + base)
    if not cells["5p"] or not cells["3p"]:
        raise ValueError("an end without rows")
    largest = max(list(cells["5p"]) + list(cells["3p"]))
    if not (1 <= k < largest and k <= 254):
        raise ValueError("K")
    out = []
    for end in ("5p", "3p"):
        rows = [cells[end].get(z, (0, 0)) for z in range(1, k + 1)]
        rows.append((sum(s for z, (s, b) in cells[end].items() if z > k), sum(b for z, (s, b) in cells[end].items() if z > k)))
        rated = []
        for z, (s, b) in enumerate(rows):
            if b == 0 and z == 0:
                raise ValueError("position 1 without data")
            rated.append((s, b, s / b if b else rated[-1][2]))
        out.append(rated)
    return out[0], out[1]


def rates(rows):
    return [r for _, _, r in rows]


# ---------------------------------------------------------------------- the error model
def p_obs(obs, true, e, ct, ga):
    """P(observed base | true allele), the issue's table."""
    if true in (A, T):
        return 1 - e if obs == true else e / 3
    if true == C:
        return {C: (1 - ct) * (1 - e) + ct * (e / 3), T: ct * (1 - e) + (1 - ct) * (e / 3)}.get(obs, e / 3)
    return {G: (1 - ga) * (1 - e) + ga * (e / 3), A: ga * (1 - e) + (1 - ga) * (e / 3)}.get(obs, e / 3)


def real_terms(obs, q, ct, ga):
    """The ten genotypes' log likelihoods of one observed base as reals."""
    e = min(0.75, 10 ** (-q / 10))
    return [math.log(p_obs(obs, a1, e, ct, ga) / 2 + p_obs(obs, a2, e, ct, ga) / 2) for a1, a2 in PAIRS]


def channel_terms(r, q):
    """The nine terms of the channel form, evaluated in the order the issue writes them: what the table holds."""
    e = min(0.75, 10 ** (-q / 10))
    pss = (1 - r) * (1 - e) + r * (e / 3)
    pst = r * (1 - e) + (1 - r) * (e / 3)
    reals = [math.log(pss), math.log(pss / 2 + (e / 3) / 2), math.log(e / 3),
             math.log(1 - e), math.log(pst / 2 + (1 - e) / 2), math.log(pst), math.log((1 - e) / 2 + (e / 3) / 2), math.log(pst / 2 + (e / 3) / 2),
             math.log(e / 3)]
    return [round(math.ldexp(x, 24)) for x in reals]


def table(d5, d3):
    """[2][K + 1][94][9] of Python integers."""
    return [[[channel_terms(r, q) for q in range(94)] for r in rates(rows)] for rows in (d5, d3)]


def which_term(obs, a1, a2):
    """The place among the nine of the observed base's term under a1 a2, from the issue's two lists."""
    s, t = (C, T) if obs in (C, T) else (G, A)
    genotype = sorted((a1, a2))
    if obs == s:
        return 0 if genotype == [s, s] else 1 if s in genotype else 2
    if genotype == [t, t]:
        return 3
    if genotype == sorted((s, t)):
        return 4
    if genotype == [s, s]:
        return 5
    if t in genotype:
        return 6
    if s in genotype:
        return 7
    return 8


def ten_terms(obs, q, ct, ga):
    """The ten integers a pair adds: the channel form's entries of its rate, placed by genotype.  ``test_channel_form_is_the_model``
    holds them to ``real_terms``."""
    nine = channel_terms(ct if obs in (C, T) else ga, q)
    return [nine[which_term(obs, a1, a2)] for a1, a2 in PAIRS]


# ---------------------------------------------------------------------- the pairs
def distances(flag, cigar, l_seq, q):
    """(z5, z3) of SEQ index q: query bases from the molecule's 5' and 3' end, [qs, qe) as the windows of --pileup-mask-ends have
    them; without a query qs = qe = 0; below 1: 1."""
    qs, qe = PR.query_range(cigar, l_seq)
    if qe <= qs:
        qs = qe = 0
    left, right = max(1, q - qs + 1), max(1, qe - q)
    return (right, left) if flag & 0x10 else (left, right)


def brute(records, n_libraries, lengths, sites, d5, d3, k5=0, k3=0, min_qual=0, noqual=30):
    """``d5``, ``d3``: the K + 1 rates of either end -> (sums: a list per site of 20 Python integers, [strand][genotype]; dict of
    the pairs added and those of them from records without qualities)."""
    n_rows = len(d5)
    assert len(d3) == n_rows
    index = {site: g for g, site in enumerate(sites)}
    by_tid = {}
    for t, p in sites:
        by_tid.setdefault(t, set()).add(p)
    sums = [[0] * 20 for _ in sites]
    counts = dict(added=0, without_qualities=0)
    cache = {}
    for record in records:
        flag, lib, tid, pos, cigar, seq, qual = record
        if PR.classify(flag, lib, tid, pos, cigar, n_libraries, lengths) != PR.COUNTED:
            continue
        where = {at: q for at, q, op in PR.columns(pos, cigar) if at is not None and q is not None}
        for p, (cls, quality, with_qual) in GR.pair_qualities(record, by_tid.get(tid, set()), k5, k3, min_qual, noqual).items():
            z5, z3 = distances(flag, cigar, len(seq), where[p])
            r5, r3 = d5[min(z5, n_rows) - 1], d3[min(z3, n_rows) - 1]
            ct, ga = (r3, r5) if flag & 0x10 else (r5, r3)
            key = (cls & 3, quality, ct, ga)
            if key not in cache:
                cache[key] = ten_terms(cls & 3, quality, ct, ga)
            row = sums[index[(tid, p)]]
            for g, term in enumerate(cache[key]):
                row[10 * (cls >> 2) + g] += term
            counts["added"] += 1
            counts["without_qualities"] += 0 if with_qual else 1
    return sums, counts


def likelihoods(row, counters, alleles=None, single_strand=False):
    """The ten values (the best one 0), the index of the best and Bases of one site from its 20 sums and its counters."""
    eligible = [s for s, ok in enumerate(GR.strands(alleles, single_strand)) if ok]
    bases = sum(int(counters[4 * s + b]) for s in eligible for b in range(4))
    if bases == 0:
        return [0] * 10, 0, 0
    logl = [sum(int(row[10 * s + g]) for s in eligible) for g in range(10)]
    top = max(logl)
    return [v - top for v in logl], logl.index(top), bases


def all_likelihoods(sums, counters, alleles=None, single_strand=False):
    out = [likelihoods(sums[g], counters[g], None if alleles is None else alleles[g], single_strand) for g in range(len(sums))]
    return np.array([o[0] for o in out], np.int64).reshape(-1, 10), [o[1] for o in out], [o[2] for o in out]


# ---------------------------------------------------------------------- the files
def profile_text(d5, d3):
    k = len(d5) - 1
    rows = ["End\tPosition\tSubstitutions\tBases\tRate"]
    for end, ones in (("5p", d5), ("3p", d3)):
        rows += ["%s\t%s\t%d\t%d\t%s" % (end, z + 1 if z < k else ">%d" % k, s, b, "%.15g" % r) for z, (s, b, r) in enumerate(ones)]
    return "\n".join(rows) + "\n"


def log_line(path, d5, d3):
    return ("Pileup damage profile: %s, %d positions; 5p C>T %.6g at position 1, tail %.6g; 3p G>A %.6g, tail %.6g"
            % (path, len(d5) - 1, d5[0][2], d5[-1][2], d3[0][2], d3[-1][2]))


def misincorporation_text(rows5, rows3, libraries=(("s", "lib"),), strands="+-", comments=False):
    """A misincorporation.txt whose C / C>T columns of the 5p rows and G / G>A columns of the 3p rows sum to ``rows5`` and
    ``rows3`` ([(substitutions, bases)] from position 1): the first library and strand take the remainder of an even split."""
    head = ["Sample", "Library", "End", "Std", "Pos", "A", "C", "G", "T", "Total", "G>A", "C>T", "A>G", "T>C"]
    if comments:
        head = ["Chr"] + head[2:]
    out = ["# table produced by mapDamage", "# using mapped file x.bam", ""] if comments else []
    out.append("\t".join(head))
    parts = [(lib, s) for lib in libraries for s in strands]
    for end, rows in (("5p", rows5), ("3p", rows3)):
        for n, (lib, strand) in enumerate(parts):
            for z, (sub, base) in enumerate(rows, 1):
                # (substitutions and the other bases split apart, so that no row has more substitutions than bases)
                share_s = sub // len(parts)
                share_b = share_s + (base - sub) // len(parts)
                if n == 0:
                    share_b, share_s = base - share_b * (len(parts) - 1), sub - share_s * (len(parts) - 1)
                c, g, ct, ga = (share_b, 7, share_s, 1) if end == "5p" else (9, share_b, 2, share_s)
                lead = ["chr1"] if comments else list(lib)
                out.append("\t".join(lead + [end, strand, str(z), "11", str(c), str(g), "13", str(31 + c + g), str(ga), str(ct), "0", "1"]))
    return "\n".join(out) + "\n"
