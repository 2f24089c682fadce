"""--depth, restated by brute force as the issue words the rule (no line of csrc/mdx_depth_key.h): per record whether it is
counted, outside or ignored, its covered intervals, then ``depth[tid][s:e] += 1`` in numpy and from that the per-sequence
numbers, the histogram and the runs.  The CPU tests hold the header's host build to it, the GPU tests the device stage and the
command line's files."""

import numpy as np

COVER_OPS = (0, 7, 8)              # M = X
SKIP_OPS = (2, 3)                  # D N
IGNORED, COUNTED, OUTSIDE = 0, 1, 2
BINS = 1024


def classify(flag, lib, tid, pos, cigar, n_libraries, lengths):
    """One of IGNORED, COUNTED, OUTSIDE; ``cigar``: [(op, length), ...], ``lengths``: of the reference's sequences."""
    if flag & 0xF04 or lib >= n_libraries:
        return IGNORED
    if not 0 <= tid < len(lengths) or pos < 0:
        return OUTSIDE
    span = sum(ln for op, ln in cigar if op in COVER_OPS + SKIP_OPS)
    if span < 1 or pos + span > lengths[tid]:
        return OUTSIDE
    return COUNTED


def intervals(pos, cigar):
    """The covered intervals [s, e) of a counted record: M, = and X cover, D and N part two intervals, everything else — and
    an operation of length 0 — is as if it were not there."""
    out, at = [], pos
    open_ = None
    for op, ln in cigar:
        if ln == 0:
            continue
        if op in COVER_OPS:
            open_ = at if open_ is None else open_
            at += ln
        elif op in SKIP_OPS:
            if open_ is not None:
                out.append((open_, at))
                open_ = None
            at += ln
    if open_ is not None:
        out.append((open_, at))
    return out


def runs_of(depth):
    """``depth``: an array per sequence -> (tid, start, end, depth) of the maximal runs of equal depth > 0, in reference order."""
    tid, start, end, value = [], [], [], []
    for t, d in enumerate(depth):
        if not len(d):
            continue
        cut = np.flatnonzero(np.diff(d) != 0) + 1
        s = np.concatenate([[0], cut])
        e = np.concatenate([cut, [len(d)]])
        keep = d[s] > 0
        tid.append(np.full(int(keep.sum()), t, np.int32))
        start.append(s[keep])
        end.append(e[keep])
        value.append(d[s][keep])
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    return cat(tid, np.int32), cat(start, np.int64), cat(end, np.int64), cat(value, np.uint32)


def brute(records, n_libraries, lengths):
    """``records``: (flag, lib, tid, pos, cigar) -> dict: ``depth`` (an int64 array per sequence), ``per_contig`` uint64
    [sequences][4] = records, covered, aligned, max, ``hist`` uint64 [1024], ``counts`` = counted, outside, intervals, runs of
    depth > 0, ``runs`` = (tid, start, end, depth), ``kinds``."""
    lengths = [int(x) for x in lengths]
    depth = [np.zeros(n, np.int64) for n in lengths]
    per_contig = np.zeros((len(lengths), 4), np.uint64)
    kinds, n_iv = [], 0
    for flag, lib, tid, pos, cigar in records:
        kind = classify(flag, lib, tid, pos, cigar, n_libraries, lengths)
        kinds.append(kind)
        if kind != COUNTED:
            continue
        per_contig[tid, 0] += 1
        for s, e in intervals(pos, cigar):
            depth[tid][s:e] += 1
            n_iv += 1
    hist = np.zeros(BINS, np.uint64)
    for t, d in enumerate(depth):
        per_contig[t, 1] = int((d > 0).sum())
        per_contig[t, 2] = int(d.sum())
        per_contig[t, 3] = int(d.max()) if len(d) else 0
        hist += np.bincount(np.minimum(d, BINS - 1), minlength=BINS).astype(np.uint64)
    runs = runs_of(depth)
    counts = dict(counted=kinds.count(COUNTED), outside=kinds.count(OUTSIDE), intervals=n_iv, runs=len(runs[0]))
    return dict(depth=depth, per_contig=per_contig, hist=hist, counts=counts, runs=runs, kinds=kinds)


def g15(x):
    return "%.15g" % x


def coverage_text(names, lengths, per_contig):
    """coverage.tsv as the issue words it."""
    rows = ["Sequence\tLength\tReads\tCovered\tBreadth\tAlignedBases\tMeanDepth\tMaxDepth"]
    table = [[int(x) for x in row] for row in per_contig]
    total = [sum(r[q] for r in table) for q in range(3)] + [max([r[3] for r in table] + [0])]
    for name, length, (reads, covered, aligned, deepest) in list(zip(names, lengths, table)) + [("*", sum(lengths), total)]:
        rows.append("\t".join([name, str(length), str(reads), str(covered), g15(covered / length) if length else "NaN", str(aligned),
                               g15(aligned / length) if length else "NaN", str(deepest)]))
    return "\n".join(rows) + "\n"


def histogram_text(hist):
    return "Depth\tBases\n" + "".join("%s\t%d\n" % (">=1023" if d == BINS - 1 else str(d), int(n)) for d, n in enumerate(hist) if n)


def bedgraph_text(names, runs):
    return "".join("%s\t%d\t%d\t%d\n" % (names[t], s, e, d) for t, s, e, d in zip(*(a.tolist() for a in runs)))
