"""--pileup-sites: the list of sites read and held to the input's header, and the files written from what
``DamageEngine.pileup_finish`` delivers.  Text only: the counters, the reference's letters, the depths and the calls are the
device's (csrc/mdx_pileup.hip, the rule: csrc/mdx_pileup_key.h), nothing is counted or drawn here.  --pileup-likelihoods: the
table of the model's terms, which the device only adds, and the files written from ``DamageEngine.pileup_likelihoods_finish``;
nothing of the likelihoods is added or reduced here either."""
import gzip
import math
import os
import re
import tempfile

import numpy as np

from .depth import _replace_with, _umask

COUNTERS = ("A+", "C+", "G+", "T+", "A-", "C-", "G-", "T-", "Deletions", "LowQual", "Other", "Masked")
PILEUP_HEADER = "Sequence\tPosition\tId\tRef\tAlt\tRefBase\t" + "\t".join(COUNTERS) + "\tDepth"
SUMMARY_HEADER = ("SitesFile\tMinBaseQual\tMaskEnds\tCall\tSeed\tMinDepth\tSingleStrandMode\tSites\tCovered\tCalled\tSumDepth\tMeanDepth\t"
                  "RecordsCounted\tRecordsOutside\tRecordsOverASite\tPairs\tDeletions\tLowQual\tOther\tMasked\n")
CALLS = ("random", "majority", "none")
BASES = "ACGT"
PILEUP_CHUNK = 1 << 16        # rows formatted at a time


class Sites:
    """The sites in (tid, position) order: ``tid`` int32, ``pos`` int32 0-based, ``off`` int64 [sequences + 1] — a sequence's
    slice —, ``alleles`` uint8 [sites][2] (0 .. 3 for A C G T) or None, ``ids`` (a list, ``.`` where the file gave none)."""

    def __init__(self, tid, pos, off, alleles, ids):
        self.tid, self.pos, self.off, self.alleles, self.ids = tid, pos, off, alleles, ids

    def __len__(self):
        return len(self.pos)


def parse_mask_ends(text):
    """--pileup-mask-ends, ``K5[,K3]``, as ``(k5, k3)``: one number means both ends, 0..255 each (None: 0,0).  ValueError
    otherwise."""
    if text is None:
        return 0, 0
    entries = [entry.strip() for entry in str(text).split(",")]
    if len(entries) > 2:
        raise ValueError("%r has more than two numbers (K5[,K3])" % str(text))
    values = []
    for entry in entries:
        if not re.fullmatch(r"[0-9]+", entry):
            raise ValueError("%r is not a number of bases (K5[,K3], 0..255 each)" % entry)
        if int(entry) > 255:
            raise ValueError("%s is above 255 bases" % entry)
        values.append(int(entry))
    return tuple(values) if len(values) == 2 else (values[0], values[0])


def first_line_has_alleles(lines):
    """Does the first line of the list that is neither empty nor a comment bring alleles?  None: there is no such line."""
    for line in lines:
        line = line.rstrip("\r\n")
        if line and not line.startswith("#"):
            return len(line.split("\t")) >= 4
    return None


def parse_sites(lines, names, lengths, source="the sites file"):
    """``lines`` of ``sequence<TAB>position[<TAB>ref<TAB>alt[<TAB>id]]`` -> ``Sites``; ``position`` is 1-based.  ``#`` lines and
    empty lines are skipped, the order is free.  ValueError names the line of anything else: fewer than two columns, a position
    that is no integer, below 1 or beyond its sequence's length, a sequence the header lacks, ref or alt that is not one of A C
    G T, ref == alt, a ref without alt, lines with alleles beside lines without, a site named twice, an empty list."""
    tid_of = {}
    for t, name in enumerate(names):
        tid_of.setdefault(name, t)
    tids, positions, refs, alts, ids, where = [], [], [], [], [], []
    with_alleles = without_alleles = None
    for number, line in enumerate(lines, 1):
        line = line.rstrip("\r\n")
        if not line or line.startswith("#"):
            continue
        fields = line.split("\t")
        if len(fields) < 2:
            raise ValueError("%s, line %d: fewer than two columns (sequence<TAB>position[<TAB>ref<TAB>alt[<TAB>id]])" % (source, number))
        t = tid_of.get(fields[0])
        if t is None:
            raise ValueError("%s, line %d: sequence '%s' is not in the input's header" % (source, number, fields[0]))
        if not re.fullmatch(r"[+-]?[0-9]+", fields[1]):
            raise ValueError("%s, line %d: position '%s' is not an integer" % (source, number, fields[1]))
        position = int(fields[1])
        if position < 1:
            raise ValueError("%s, line %d: position %d is below 1 (positions are 1-based)" % (source, number, position))
        if position > int(lengths[t]):
            raise ValueError("%s, line %d: position %d lies beyond the %d bases of sequence '%s'" % (source, number, position, int(lengths[t]), fields[0]))
        if len(fields) == 3:
            raise ValueError("%s, line %d: a ref without an alt" % (source, number))
        if len(fields) >= 4:
            for what, allele in (("ref", fields[2]), ("alt", fields[3])):
                if allele not in ("A", "C", "G", "T"):
                    raise ValueError("%s, line %d: %s '%s' is not exactly one of A C G T" % (source, number, what, allele))
            if fields[2] == fields[3]:
                raise ValueError("%s, line %d: ref and alt are both '%s'" % (source, number, fields[2]))
            with_alleles = number if with_alleles is None else with_alleles
            refs.append(BASES.index(fields[2]))
            alts.append(BASES.index(fields[3]))
        else:
            without_alleles = number if without_alleles is None else without_alleles
        if with_alleles is not None and without_alleles is not None:
            raise ValueError("%s: line %d has alleles and line %d has none; either every site brings ref and alt or none does"
                             % (source, with_alleles, without_alleles))
        tids.append(t)
        positions.append(position - 1)
        ids.append(fields[4] if len(fields) >= 5 and fields[4] else ".")
        where.append(number)
    if not tids:
        raise ValueError("%s holds no site" % source)
    tid, pos = np.array(tids, np.int32), np.array(positions, np.int32)
    order = np.lexsort((pos, tid))          # (stable: of two equal sites the earlier line first)
    tid, pos = tid[order], pos[order]
    same = np.flatnonzero((tid[1:] == tid[:-1]) & (pos[1:] == pos[:-1]))
    if len(same):
        a, b = int(order[same[0]]), int(order[same[0] + 1])
        raise ValueError("%s: lines %d and %d name the same site, %s:%d" % (source, where[a], where[b], names[int(tid[same[0]])], int(pos[same[0]]) + 1))
    off = np.zeros(len(names) + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(tid, minlength=len(names)))
    alleles = np.stack([np.array(refs, np.uint8)[order], np.array(alts, np.uint8)[order]], axis=1) if with_alleles is not None else None
    return Sites(tid, pos, off, alleles, [ids[int(k)] for k in order])


def read_sites(path, names, lengths):
    with open(path, "r") as handle:
        return parse_sites(handle, names, lengths, source="--pileup-sites %s" % path)


def _letters(a):
    return np.asarray(a, "S1").astype("U1").tolist()


def pileup_chunks(names, sites, counters, refbase, call, depth, with_call=True, chunk=PILEUP_CHUNK):
    """pileup.tsv as bytes, a chunk of rows at a time: a line per site in (tid, position) order, the position 1-based; ``Id``,
    ``Ref`` and ``Alt`` are ``.`` where the list gave none; no ``Call`` column without ``with_call``."""
    yield (PILEUP_HEADER + ("\tCall\n" if with_call else "\n")).encode()
    counters = np.asarray(counters, np.uint32).reshape(-1, len(COUNTERS))
    for lo in range(0, len(sites), chunk):
        hi = min(len(sites), lo + chunk)
        tid, pos = sites.tid[lo:hi].tolist(), (sites.pos[lo:hi].astype(np.int64) + 1).tolist()
        if sites.alleles is not None:
            ref, alt = ([BASES[b] for b in sites.alleles[lo:hi, q].tolist()] for q in (0, 1))
        else:
            ref = alt = ["."] * (hi - lo)
        rows = counters[lo:hi].tolist()
        letters, calls, depths = _letters(refbase[lo:hi]), _letters(call[lo:hi]), np.asarray(depth[lo:hi]).tolist()
        out = []
        for k in range(hi - lo):
            out.append("%s\t%d\t%s\t%s\t%s\t%s\t%s\t%d%s\n" % (names[tid[k]], pos[k], sites.ids[lo + k], ref[k], alt[k], letters[k],
                                                             "\t".join(map(str, rows[k])), depths[k], "\t" + calls[k] if with_call else ""))
        yield "".join(out).encode()


def write_pileup(path, names, sites, counters, refbase, call, depth, with_call=True):
    """pileup.tsv under a temporary name in ``path``'s directory, moved into place at the end; any failure removes it."""
    _replace_with(path, pileup_chunks(names, sites, counters, refbase, call, depth, with_call))


def totals(counters, call, depth, with_call=True):
    """(sites, covered, called, sum of depths, [Deletions, LowQual, Other, Masked]) of the whole list."""
    counters = np.asarray(counters, np.uint32).reshape(-1, len(COUNTERS))
    depth = np.asarray(depth, np.int64)
    called = int(np.isin(np.asarray(call, "S1"), np.array([b"A", b"C", b"G", b"T"], "S1")).sum()) if with_call else 0
    return len(depth), int((depth >= 1).sum()), called, int(depth.sum()), [int(x) for x in counters[:, 8:].sum(axis=0, dtype=np.uint64)]


def summary_text(options, counters, call, depth, counts):
    """pileup_summary.tsv: one line of the option values and the totals.  ``options``: a dict of path, min_basequal, mask_ends,
    call, seed, min_depth, single_strand."""
    with_call = options["call"] != "none"
    n, covered, called, total, rest = totals(counters, call, depth, with_call)
    return SUMMARY_HEADER + "%s\t%d\t%d,%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
        options["path"], options["min_basequal"], options["mask_ends"][0], options["mask_ends"][1], options["call"], options["seed"],
        options["min_depth"], int(bool(options["single_strand"])), n, covered, called, total, "%.15g" % (total / n) if n else "NaN",
        counts["counted"], counts["outside"], counts["over_a_site"], counts["pairs"], rest[0], rest[1], rest[2], rest[3])


def log_line(options, counters, call, depth, counts):
    with_call = options["call"] != "none"
    n, covered, called, total, _ = totals(counters, call, depth, with_call)
    how = "%s, seed %d" % (options["call"], options["seed"]) if with_call else "none"
    return ("Pileup: %d sites, %d covered (%s %%), %d called (%s), mean depth %s at sites; %d of %d records over a site; %d records "
            "outside their sequence" % (n, covered, "%.4g" % (100.0 * covered / n) if n else "NaN", called, how,
                                        "%.6g" % (total / n) if n else "NaN", counts["over_a_site"], counts["counted"], counts["outside"]))


def off_build(sites, refbase):
    """The sites whose reference letter is neither their ref nor their alt — the usual sign of a panel made for another genome
    build; 0 without alleles."""
    if sites.alleles is None:
        return 0
    letter = np.asarray(refbase, "S1").view(np.uint8)
    table = np.frombuffer(BASES.encode(), np.uint8)
    return int(((letter != table[sites.alleles[:, 0]]) & (letter != table[sites.alleles[:, 1]])).sum())


# ---------------------------------------------------------------------- --pileup-likelihoods
GENOTYPES = ("AA", "AC", "AG", "AT", "CC", "CG", "CT", "GG", "GT", "TT")
LIKELIHOODS_HEADER = "Sequence\tPosition\tId\tRef\tAlt\tBases\t" + "\t".join(GENOTYPES) + "\tBest\n"
LIKELIHOODS_SUMMARY_HEADER = "SitesFile\tMinBaseQual\tMaskEnds\tSingleStrandMode\tNoQualQuality\tSites\tSitesWithBases\tBaseObservations\tWithoutQualities\n"
BEAGLE_HEADER = "marker\tallele1\tallele2\tInd0\tInd0\tInd0\n"
GL_QUALITIES, GL_SCALE_BITS = 94, 24
GL_UNIT = float(1 << GL_SCALE_BITS)


def likelihood_table():
    """int64 [94][3], per quality q the terms HOM, HET, NO of GATK's model (ANGSD -GL 2) as ``round(term * 2^24)``: with e =
    min(0.75, 10^(-q/10)) the log likelihood of an observed base b under a genotype bb, under a heterozygous one that holds b,
    under any other.  Python doubles in exactly this order, so that every build of the table is the same one; the device only
    adds its entries (csrc/mdx_pileup_key.h)."""
    rows = []
    for q in range(GL_QUALITIES):
        e = min(0.75, 10.0 ** (-q / 10.0))
        hom = math.log(1.0 - e)
        het = math.log((1.0 - e) / 2.0 + e / 6.0)
        no = math.log(e / 3.0)
        rows.append([round(math.ldexp(x, GL_SCALE_BITS)) for x in (hom, het, no)])
    table = np.array(rows, np.int64)
    # (a record adds at most one term to a sum and fewer than 2^31 records are added: no sum leaves its int64)
    assert int(np.abs(table).max()) << 31 < 1 << 63
    return table


def genotype_index(a, b):
    """The place of the genotype of the bases ``a`` and ``b`` (0 .. 3) in GENOTYPES."""
    a, b = np.minimum(a, b), np.maximum(a, b)           # (numbers or arrays of them)
    return 4 * a - a * (a - 1) // 2 + (b - a)


def likelihoods_chunks(names, sites, gl, best, bases, chunk=PILEUP_CHUNK):
    """pileup_likelihoods.tsv as bytes, a chunk of rows at a time: a line per site in the order of pileup.tsv; a genotype's value
    is ``gl / 2^24 / ln 10``, the log10 of its likelihood over the best one's; ``Best`` is ``.`` where no base was taken."""
    yield LIKELIHOODS_HEADER.encode()
    gl = np.asarray(gl, np.int64).reshape(-1, len(GENOTYPES))
    row_format = "%s\t%d\t%s\t%s\t%s\t%d" + "\t%.6f" * len(GENOTYPES) + "\t%s\n"
    for lo in range(0, len(sites), chunk):
        hi = min(len(sites), lo + chunk)
        tid, pos = sites.tid[lo:hi].tolist(), (sites.pos[lo:hi].astype(np.int64) + 1).tolist()
        if sites.alleles is not None:
            ref, alt = ([BASES[b] for b in sites.alleles[lo:hi, q].tolist()] for q in (0, 1))
        else:
            ref = alt = ["."] * (hi - lo)
        values = (gl[lo:hi].astype(np.float64) / GL_UNIT / math.log(10.0)).tolist()
        n, first = np.asarray(bases[lo:hi]).tolist(), np.asarray(best[lo:hi]).tolist()
        out = []
        for k in range(hi - lo):
            out.append(row_format % ((names[tid[k]], pos[k], sites.ids[lo + k], ref[k], alt[k], n[k]) + tuple(values[k])
                                     + (GENOTYPES[first[k]] if n[k] else ".",)))
        yield "".join(out).encode()


def write_likelihoods(path, names, sites, gl, best, bases):
    """pileup_likelihoods.tsv under a temporary name in ``path``'s directory, moved into place at the end."""
    _replace_with(path, likelihoods_chunks(names, sites, gl, best, bases))


def beagle_chunks(names, sites, gl, bases, chunk=PILEUP_CHUNK):
    """The BEAGLE GL file of ``angsd -doGlf 2`` as bytes: per site ``<sequence>_<position>``, ref and alt as 0 1 2 3 for A C G
    T, and the likelihoods of ref/ref, ref/alt and alt/alt, ``exp(gl / 2^24)`` over their sum — a third each where no base was
    taken.  The list brings alleles."""
    yield BEAGLE_HEADER.encode()
    gl = np.asarray(gl, np.int64).reshape(-1, len(GENOTYPES))
    for lo in range(0, len(sites), chunk):
        hi = min(len(sites), lo + chunk)
        ref, alt = sites.alleles[lo:hi, 0].astype(np.int64), sites.alleles[lo:hi, 1].astype(np.int64)
        rows = np.arange(hi - lo)
        three = np.stack([gl[lo:hi][rows, genotype_index(x, y)] for x, y in ((ref, ref), (ref, alt), (alt, alt))], axis=1)
        # (over the largest of the three, which leaves the quotients as they are: at a deep site whose bases are neither allele
        # all three are far below the best genotype and would underflow to 0 / 0)
        like = np.exp((three - three.max(axis=1, keepdims=True)).astype(np.float64) / GL_UNIT)
        like /= like.sum(axis=1, keepdims=True)
        like[np.asarray(bases[lo:hi]) == 0] = 1.0 / 3.0
        tid, pos = sites.tid[lo:hi].tolist(), (sites.pos[lo:hi].astype(np.int64) + 1).tolist()
        ref, alt, like = ref.tolist(), alt.tolist(), like.tolist()
        yield "".join("%s_%d\t%d\t%d\t%.6f\t%.6f\t%.6f\n" % ((names[tid[k]], pos[k], ref[k], alt[k]) + tuple(like[k])) for k in range(hi - lo)).encode()


def write_beagle(path, names, sites, gl, bases):
    """--pileup-beagle PATH under a temporary name in its directory, moved into place at the end; any failure removes it.  A
    path that ends in ``.gz`` is gzip with a zero mtime and no name, so the same run writes the same bytes."""
    path = os.path.abspath(str(path))
    if not path.endswith(".gz"):
        _replace_with(path, beagle_chunks(names, sites, gl, bases))
        return
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(path))
    try:
        with os.fdopen(fd, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as out:
            for text in beagle_chunks(names, sites, gl, bases):
                out.write(text)
        os.chmod(tmp, 0o666 & ~_umask())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def likelihoods_summary_text(options, bases, counts):
    """pileup_likelihoods_summary.tsv: one line of the option values, the sites, those with at least one base, the base
    observations and those of them from records without qualities.  ``options``: summary_text's and noqual_quality."""
    bases = np.asarray(bases, np.int64)
    return LIKELIHOODS_SUMMARY_HEADER + "%s\t%d\t%d,%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
        options["path"], options["min_basequal"], options["mask_ends"][0], options["mask_ends"][1], int(bool(options["single_strand"])),
        options["noqual_quality"], len(bases), int((bases >= 1).sum()), counts["added"], counts["without_qualities"])


def likelihoods_log_line(options, bases, counts):
    bases = np.asarray(bases, np.int64)
    return ("Pileup likelihoods: %d sites, %d with bases, %d base observations (%d from records without qualities, taken at %d)"
            % (len(bases), int((bases >= 1).sum()), counts["added"], counts["without_qualities"], options["noqual_quality"]))
