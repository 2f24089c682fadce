"""--depth: the files written from what ``DamageEngine.depth_finish`` / ``depth_runs`` deliver.  Text only: the numbers are
the device's (csrc/mdx_depth.hip), nothing is counted here."""
import os
import tempfile

import numpy as np

COVERAGE_HEADER = "Sequence\tLength\tReads\tCovered\tBreadth\tAlignedBases\tMeanDepth\tMaxDepth\n"
HISTOGRAM_HEADER = "Depth\tBases\n"
BEDGRAPH_CHUNK = 1 << 20      # rows formatted at a time


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
    path = os.path.abspath(str(path))
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(path))
    try:
        with os.fdopen(fd, "wb") as out:
            for text in bedgraph_chunks(names, tid, start, end, depth):
                out.write(text)
        os.chmod(tmp, 0o666 & ~_umask())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def _umask():
    mask = os.umask(0)
    os.umask(mask)
    return mask
