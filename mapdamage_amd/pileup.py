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


# ---------------------------------------------------------------------- --pileup-damage-profile
GLD_TERMS, GLD_MAX_POSITIONS, GLD_DEFAULT_POSITIONS = 9, 254, 20
DAMAGE_PROFILE_HEADER = "End\tPosition\tSubstitutions\tBases\tRate\n"
PROFILE_ENDS = (("5p", "C", "C>T"), ("3p", "G", "G>A"))         # the end, its base column and its substitution column


class ProfileError(ValueError):
    """A misincorporation.txt that --pileup-damage-profile cannot take; the message names the file (and the line)."""


class DamageProfile:
    """``positions`` K; ``ends``: per end of PROFILE_ENDS its K + 1 rows ``(substitutions, bases, rate)``, the last the pooled
    tail of the positions K + 1 .. ``largest``; a row without bases has the rate of the nearest row in front of it."""

    def __init__(self, path, positions, largest, ends):
        self.path, self.positions, self.largest, self.ends = path, positions, largest, ends

    def rates(self, end):
        return [row[2] for row in self.ends[end]]


def parse_damage_profile(lines, positions=GLD_DEFAULT_POSITIONS, source="the damage profile"):
    """A misincorporation.txt, this project's or mapDamage's: ``#`` lines and empty lines skipped, the first line left is the
    header, the columns End, Pos, C, G, C>T and G>A found by name; C>T over C of the 5p rows and G>A over G of the 3p rows,
    summed over samples, libraries and strands per position.  Raises ProfileError."""
    sums = ({}, {})                 # per end {position: [substitutions, bases]}
    column = None
    for number, line in enumerate(lines, 1):
        line = line.rstrip("\r\n")
        if not line.strip() or line.startswith("#"):
            continue
        fields = line.split("\t")
        if column is None:
            names = {name: i for i, name in enumerate(fields)}
            missing = [name for name in ("End", "Pos", "C", "G", "C>T", "G>A") if name not in names]
            if missing:
                raise ProfileError("%s, line %d: the header lacks the column%s %s" % (source, number, "s" if len(missing) > 1 else "", ", ".join(missing)))
            column = names
            continue
        if len(fields) <= max(column[name] for name in ("End", "Pos", "C", "G", "C>T", "G>A")):
            raise ProfileError("%s, line %d: %d fields, fewer than the header's" % (source, number, len(fields)))
        end = fields[column["End"]]
        if end not in ("5p", "3p"):
            raise ProfileError("%s, line %d: End is %r, neither 5p nor 3p" % (source, number, end))
        numbers = {}
        for name in ("Pos", "C", "G", "C>T", "G>A"):
            text = fields[column[name]]
            if not text.isascii() or not text.isdigit():
                raise ProfileError("%s, line %d: %s is %r, not a non-negative integer" % (source, number, name, text))
            numbers[name] = int(text)
        if numbers["Pos"] < 1:
            raise ProfileError("%s, line %d: Pos is 0; positions count from 1" % (source, number))
        for base, sub in (("C", "C>T"), ("G", "G>A")):
            if numbers[sub] > numbers[base]:
                raise ProfileError("%s, line %d: %s is %d, above the %d of %s" % (source, number, sub, numbers[sub], numbers[base], base))
        which = 0 if end == "5p" else 1
        _, base, sub = PROFILE_ENDS[which]
        cell = sums[which].setdefault(numbers["Pos"], [0, 0])
        cell[0] += numbers[sub]
        cell[1] += numbers[base]
    if column is None:
        raise ProfileError("%s holds no header line" % source)
    for which, (end, _, _) in enumerate(PROFILE_ENDS):
        if not sums[which]:
            raise ProfileError("%s holds no %s rows" % (source, end))
    largest = max(max(sums[0]), max(sums[1]))
    if not 1 <= positions <= GLD_MAX_POSITIONS:
        raise ProfileError("--pileup-damage-positions %d: 1..%d positions" % (positions, GLD_MAX_POSITIONS))
    if positions >= largest:
        raise ProfileError("%s: --pileup-damage-positions %d needs positions beyond it for the tail, and the largest Pos is %d" % (source, positions, largest))
    ends = []
    for which, (end, base, sub) in enumerate(PROFILE_ENDS):
        rows, rate = [], None
        for z in range(1, positions + 2):
            if z <= positions:
                n_sub, n_base = sums[which].get(z, (0, 0))
            else:
                n_sub = sum(cell[0] for pos, cell in sums[which].items() if pos > positions)
                n_base = sum(cell[1] for pos, cell in sums[which].items() if pos > positions)
            if n_base:
                rate = n_sub / n_base
            elif rate is None:
                raise ProfileError("%s: no %s at position 1 of the %s rows; the profile needs the rate of the first position" % (source, base, end))
            rows.append((n_sub, n_base, rate))
        ends.append(rows)
    return DamageProfile(source, positions, largest, ends)


def read_damage_profile(path, positions=GLD_DEFAULT_POSITIONS):
    with open(path, newline="") as handle:
        return parse_damage_profile(handle, positions, str(path))


def damage_terms(r, q):
    """The nine terms of a channel with rate ``r`` at quality ``q`` as ``round(term * 2^24)``: the observed source under ss, s and
    another, no s; the observed product under tt, st, ss, t and another, s and another, neither.  Python doubles in exactly this
    order (csrc/mdx_pileup_key.h)."""
    e = min(0.75, 10.0 ** (-q / 10.0))
    pss = (1.0 - r) * (1.0 - e) + r * (e / 3.0)
    pst = r * (1.0 - e) + (1.0 - r) * (e / 3.0)
    terms = (math.log(pss),
             math.log(pss / 2.0 + (e / 3.0) / 2.0),
             math.log(e / 3.0),
             math.log(1.0 - e),
             math.log(pst / 2.0 + (1.0 - e) / 2.0),
             math.log(pst),
             math.log((1.0 - e) / 2.0 + (e / 3.0) / 2.0),
             math.log(pst / 2.0 + (e / 3.0) / 2.0),
             math.log(e / 3.0))
    return [round(math.ldexp(x, GL_SCALE_BITS)) for x in terms]


def damage_likelihood_table(profile):
    """int64 [2 ends][K + 1][94][9] for ``mdx_pileup_likelihoods_damage_begin``: ``damage_terms`` of every row's rate, end 0 the
    5p C>T rates, end 1 the 3p G>A rates."""
    plain = likelihood_table()
    for q in range(GL_QUALITIES):
        hom, het, no = plain[q].tolist()
        # (without damage the model is the plain one: a zero profile reproduces --pileup-likelihoods bit for bit)
        assert damage_terms(0.0, q) == [hom, het, no, hom, het, no, het, no, no], q
    # (rows without bases repeat the rate in front of them: a rate's rows are made once)
    rows = {rate: [damage_terms(rate, q) for q in range(GL_QUALITIES)] for rate in set(profile.rates(0) + profile.rates(1))}
    table = np.array([[rows[rate] for rate in profile.rates(end)] for end in range(2)], np.int64)
    assert table.shape == (2, profile.positions + 1, GL_QUALITIES, GLD_TERMS)
    # (every probability is at least e / 3: no term is larger in magnitude than the plain table's, and its bound holds)
    assert int(np.abs(table).max()) <= int(np.abs(plain).max()) and int(np.abs(table).max()) << 31 < 1 << 63
    return table


def damage_profile_text(profile):
    """pileup_damage_profile.tsv: a line per row of either end, the tail as ``>K``."""
    out = [DAMAGE_PROFILE_HEADER]
    for (end, _, _), rows in zip(PROFILE_ENDS, profile.ends):
        for z, (n_sub, n_base, rate) in enumerate(rows, 1):
            out.append("%s\t%s\t%d\t%d\t%s\n" % (end, str(z) if z <= profile.positions else ">%d" % profile.positions, n_sub, n_base, "%.15g" % rate))
    return "".join(out)


def damage_profile_log_line(profile):
    five, three = profile.rates(0), profile.rates(1)
    return ("Pileup damage profile: %s, %d positions; 5p C>T %.6g at position 1, tail %.6g; 3p G>A %.6g, tail %.6g"
            % (profile.path, profile.positions, five[0], five[-1], three[0], three[-1]))
