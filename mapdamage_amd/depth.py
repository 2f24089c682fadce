"""--depth: the files written from what ``DamageEngine.depth_finish`` / ``depth_runs`` deliver, and those of --depth-regions
from ``depth_regions``.  Text only: the numbers are the device's (csrc/mdx_depth.hip), nothing is counted here."""
import os
import tempfile

import numpy as np

COVERAGE_HEADER = "Sequence\tLength\tReads\tCovered\tBreadth\tAlignedBases\tMeanDepth\tMaxDepth\n"
HISTOGRAM_HEADER = "Depth\tBases\n"
BEDGRAPH_CHUNK = 1 << 20      # rows formatted at a time
REGION_COVERAGE_HEADER = "Index\tGroup\tRegions\tBases\tCovered\tBreadth\tAlignedBases\tMeanDepth\tMaxDepth\n"
REGION_HISTOGRAM_HEADER = "Index\tGroup\tDepth\tBases\n"
REGION_THRESHOLDS_HEADER = "Index\tGroup\tThreshold\tBases\tFraction\n"
REGIONS_DEPTH_HEADER = "Sequence\tStart\tEnd\tGroup\tCovered\tBreadth\tAlignedBases\tMeanDepth\tMinDepth\tMaxDepth\n"
REGIONS_DEPTH_CHUNK = 1 << 18  # rows formatted at a time
DEFAULT_THRESHOLDS = (1, 5, 10, 20)
MAX_THRESHOLDS = 32


def _ratio(a, length):
    return "%.15g" % (a / length) if length else "NaN"


def totals(lengths, per_contig):
    """(length, reads, covered, aligned, max) of the whole reference: the ``*`` line of coverage.tsv."""
    per_contig = np.asarray(per_contig, np.uint64).reshape(-1, 4)
    length = int(sum(int(x) for x in lengths))
    reads, covered, aligned = (int(per_contig[:, q].sum()) for q in range(3))
    return length, reads, covered, aligned, int(per_contig[:, 3].max()) if len(per_contig) else 0


def coverage_text(names, lengths, per_contig):
    """coverage.tsv: a line per sequence in tid order — length, counted records, covered bases, breadth = covered / length,
    aligned bases, mean depth = aligned / length, largest depth —, then ``*`` for the whole reference (its MaxDepth the largest
    of the sequences').  A sequence of length 0 has breadth and mean depth ``NaN``."""
    rows = [COVERAGE_HEADER]
    table = np.asarray(per_contig, np.uint64).reshape(-1, 4).tolist()
    for name, length, (reads, covered, aligned, deepest) in zip(names, lengths, table):
        length = int(length)
        rows.append("%s\t%d\t%d\t%d\t%s\t%d\t%s\t%d\n" % (name, length, reads, covered, _ratio(covered, length), aligned,
                                                       _ratio(aligned, length), deepest))
    length, reads, covered, aligned, deepest = totals(lengths, per_contig)
    rows.append("*\t%d\t%d\t%d\t%s\t%d\t%s\t%d\n" % (length, reads, covered, _ratio(covered, length), aligned, _ratio(aligned, length), deepest))
    return "".join(rows)


def histogram_text(hist):
    """depth_histogram.tsv: the non-empty bins, bases at depth ``d``; the last bin is written ``>=1023``."""
    hist = [int(x) for x in hist]
    last = len(hist) - 1
    return HISTOGRAM_HEADER + "".join("%s\t%d\n" % (d if d < last else ">=%d" % last, n) for d, n in enumerate(hist) if n)


def log_line(lengths, per_contig, counts):
    length, _, covered, aligned, deepest = totals(lengths, per_contig)
    return ("Depth: %d records, %d aligned bases; %d of %d reference bases covered (%s %%), mean depth %s, max %d; %d records "
            "outside their sequence" % (counts["counted"], aligned, covered, length, "%.4g" % (100.0 * covered / length) if length else "NaN",
                                        "%.6g" % (aligned / length) if length else "NaN", deepest, counts["outside"]))


def bedgraph_chunks(names, tid, start, end, depth, chunk=BEDGRAPH_CHUNK):
    """The runs as the text of ``bedtools genomecov -bg``, ``name\\tstart\\tend\\tdepth``, as bytes, a chunk of rows at a time.
    No loop over rows: a chunk is a matrix of bytes, a row per line — the name, then every number in a field as wide as the
    chunk's largest, its digits peeled off column by column — from which the padding (zero bytes: a shorter name's tail, the
    places in front of a number's first digit) is dropped at the end."""
    table = np.asarray([n.encode() for n in names] or [b""], dtype="S")
    width = table.dtype.itemsize
    table = table.view(np.uint8).reshape(-1, width)
    tid, start, end, depth = (np.asarray(a) for a in (tid, start, end, depth))
    for lo in range(0, len(tid), chunk):
        hi = min(len(tid), lo + chunk)
        columns = [a[lo:hi].astype(np.int64) for a in (start, end, depth)]
        widths = [len(str(int(c.max()))) for c in columns]
        rows = np.zeros((hi - lo, width + sum(widths) + 4), np.uint8)
        rows[:, :width] = table[tid[lo:hi]]
        at = width
        for column, digits in zip(columns, widths):
            rows[:, at] = 9                 # tab
            rest = column.copy()
            for place in range(digits - 1, -1, -1):
                digit = rest % 10
                rest //= 10
                # (a zero is written in the last place, or where digits are still to come in front of it)
                rows[:, at + 1 + place] = np.where((rest > 0) | (digit > 0) | (place == digits - 1), digit + 48, 0)
            at += 1 + digits
        rows[:, at] = 10                    # newline
        flat = rows.ravel()
        yield flat[flat != 0].tobytes()


def write_bedgraph(path, names, tid, start, end, depth):
    """The bedGraph under a temporary name in ``path``'s directory, moved into place at the end; any failure removes it."""
    _replace_with(path, bedgraph_chunks(names, tid, start, end, depth))


def _replace_with(path, chunks):
    """``chunks`` (bytes) under a temporary name in ``path``'s directory, moved into place at the end; any failure removes it."""
    path = os.path.abspath(str(path))
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(path))
    try:
        with os.fdopen(fd, "wb") as out:
            for text in chunks:
                out.write(text)
        os.chmod(tmp, 0o666 & ~_umask())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


# ---------------------------------------------------------------------- --depth-regions: by_region/
def parse_thresholds(text, bins=1024):
    """``--depth-thresholds T[,T...]`` (None: 1,5,10,20): strictly increasing integers in 1 .. bins - 2 — a depth the histogram
    still tells from the deeper ones —, at most 32.  ValueError says what is wrong."""
    if text is None:
        return list(DEFAULT_THRESHOLDS)
    try:
        values = [int(t) for t in str(text).split(",")]
    except ValueError:
        raise ValueError("--depth-thresholds %s: a comma-separated list of integers is expected" % text) from None
    if len(values) > MAX_THRESHOLDS:
        raise ValueError("--depth-thresholds: %d values, at most %d are taken" % (len(values), MAX_THRESHOLDS))
    if any(not 1 <= t <= bins - 2 for t in values):
        raise ValueError("--depth-thresholds %s: every threshold lies in 1..%d (the histogram's last bin holds every depth from "
                         "%d on)" % (text, bins - 2, bins - 1))
    if any(b <= a for a, b in zip(values, values[1:])):
        raise ValueError("--depth-thresholds %s: the thresholds must increase strictly" % text)
    return values


def _group_table(per_group):
    return np.asarray(per_group, np.uint64).reshape(-1, 4).tolist()


def region_coverage_text(groups, n_regions, per_group):
    """by_region/coverage.tsv: a line per group in groups.tsv order, ``*`` included — its regions and bases as there, covered
    bases, breadth = covered / bases, aligned bases, mean depth = aligned / bases, largest depth.  No bases: ``NaN``."""
    rows = [REGION_COVERAGE_HEADER]
    for g, (name, regions, (bases, covered, aligned, deepest)) in enumerate(zip(groups, n_regions, _group_table(per_group))):
        rows.append("%d\t%s\t%d\t%d\t%d\t%s\t%d\t%s\t%d\n" % (g, name, regions, bases, covered, _ratio(covered, bases), aligned,
                                                              _ratio(aligned, bases), deepest))
    return "".join(rows)


def region_histogram_text(groups, group_hist):
    """by_region/depth_histogram.tsv: per group the non-empty bins; the last bin is written ``>=1023``."""
    rows = [REGION_HISTOGRAM_HEADER]
    for g, (name, hist) in enumerate(zip(groups, np.asarray(group_hist, np.uint64).tolist())):
        last = len(hist) - 1
        rows += ["%d\t%s\t%s\t%d\n" % (g, name, d if d < last else ">=%d" % last, n) for d, n in enumerate(hist) if n]
    return "".join(rows)


def bases_at_least(hist, thresholds):
    """The bases at depth >= T for every threshold, from one group's histogram (its last bin holds every deeper base)."""
    tail = np.cumsum(np.asarray(hist, np.uint64)[::-1])[::-1]
    return [int(tail[t]) for t in thresholds]


def region_thresholds_text(groups, per_group, group_hist, thresholds):
    """by_region/depth_thresholds.tsv: per group and threshold the bases at depth >= T and their share of the group's bases."""
    rows = [REGION_THRESHOLDS_HEADER]
    for g, (name, (bases, _, _, _), hist) in enumerate(zip(groups, _group_table(per_group), np.asarray(group_hist, np.uint64))):
        for t, n in zip(thresholds, bases_at_least(hist, thresholds)):
            rows.append("%d\t%s\t%d\t%d\t%s\n" % (g, name, t, n, _ratio(n, bases)))
    return "".join(rows)


def regions_depth_chunks(names, groups, iv_off, iv_start, iv_end, iv_group, per_interval, chunk=REGIONS_DEPTH_CHUNK):
    """by_region/regions_depth.tsv without its header, as bytes, ``chunk`` rows at a time: a line per interval in tid order and
    then by start — the lines of ``samtools bedcov`` / ``mosdepth --by``.  No loop over rows: every column of a chunk is
    formatted as a whole and the columns are joined element by element."""
    iv_off = np.asarray(iv_off, np.int64)
    tid = np.repeat(np.arange(len(iv_off) - 1), np.diff(iv_off))
    start, end, group = np.asarray(iv_start, np.int64), np.asarray(iv_end, np.int64), np.asarray(iv_group, np.int64)
    table = np.asarray(per_interval, np.uint64).reshape(-1, 4)
    seq_names, group_names = np.asarray([str(n) for n in names] or [""]), np.asarray([str(g) for g in groups] or [""])
    fmt = np.char.mod
    for lo in range(0, len(tid), chunk):
        hi = min(len(tid), lo + chunk)
        span = (end[lo:hi] - start[lo:hi]).astype(np.float64)
        covered, aligned, shallowest, deepest = (table[lo:hi, q] for q in range(4))
        columns = [seq_names[tid[lo:hi]], fmt("%d", start[lo:hi]), fmt("%d", end[lo:hi]), group_names[group[lo:hi]], fmt("%d", covered),
                   fmt("%.15g", covered / span), fmt("%d", aligned), fmt("%.15g", aligned / span), fmt("%d", shallowest), fmt("%d", deepest)]
        rows = columns[0]
        for column in columns[1:]:
            rows = np.char.add(np.char.add(rows, "\t"), column)
        yield ("\n".join(rows.tolist()) + "\n").encode()


def region_log_line(per_group, rest_group=-1):
    """``Depth on target: ...``: the named groups summed, against the rest."""
    table = _group_table(per_group)
    rest = table.pop(rest_group)
    bases, covered, aligned = (sum(row[q] for row in table) for q in range(3))
    return ("Depth on target: %d of %d target bases covered (%s %%), mean depth %s on target, %s off target"
            % (covered, bases, "%.4g" % (100.0 * covered / bases) if bases else "NaN", "%.6g" % (aligned / bases) if bases else "NaN",
               "%.6g" % (rest[2] / rest[0]) if rest[0] else "NaN"))


def write_region_files(directory, names, groups, regions, result, thresholds):
    """The four files of --depth-regions in ``directory`` (by_region/): ``regions`` the run's ``tables.Regions``, ``result``
    what ``DamageEngine.depth_regions`` returned.  regions_depth.tsv is written under a temporary name and moved into place."""
    per_interval, per_group, group_hist = result
    n_regions = np.bincount(np.asarray(regions.iv_group, np.int64), minlength=len(groups)).tolist()
    (directory / "coverage.tsv").write_text(region_coverage_text(groups, n_regions, per_group))
    (directory / "depth_histogram.tsv").write_text(region_histogram_text(groups, group_hist))
    (directory / "depth_thresholds.tsv").write_text(region_thresholds_text(groups, per_group, group_hist, thresholds))

    def chunks():
        yield REGIONS_DEPTH_HEADER.encode()
        yield from regions_depth_chunks(names, groups, regions.iv_off, regions.iv_start, regions.iv_end, regions.iv_group, per_interval)
    _replace_with(directory / "regions_depth.tsv", chunks())


def _umask():
    mask = os.umask(0)
    os.umask(mask)
    return mask
