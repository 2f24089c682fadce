"""--depth-regions, restated by brute force as the issue words it: the per-base depths of tests/depth_rule.brute, sliced by
interval in numpy.  Base ``p`` of sequence ``t`` belongs to interval ``k`` of ``t`` iff ``iv_start[k] <= p < iv_end[k]``, and to
the rest otherwise.  The GPU tests hold ``DamageEngine.depth_regions`` and the command line's four files to it."""

import numpy as np

BINS = 1024


def binned(d):
    return np.bincount(np.minimum(d, BINS - 1), minlength=BINS).astype(np.uint64)


def brute(depth, iv_off, iv_start, iv_end, iv_group, n_groups, rest_group=None):
    """``depth``: an int64 array per sequence (``depth_rule.brute(...)["depth"]``); the intervals of sequence ``t`` are
    ``iv_off[t]:iv_off[t + 1]`` of the three columns.  -> ``per_interval`` uint64 [intervals][4] = covered, aligned, min, max;
    ``per_group`` uint64 [groups][4] = bases, covered, aligned, max; ``group_hist`` uint64 [groups][1024]."""
    rest_group = n_groups - 1 if rest_group is None else rest_group
    n_iv = len(iv_start)
    per_interval = np.zeros((n_iv, 4), np.uint64)
    per_group = np.zeros((n_groups, 4), np.uint64)
    group_hist = np.zeros((n_groups, BINS), np.uint64)

    def take(g, d):
        per_group[g, 0] += len(d)
        per_group[g, 1] += int((d > 0).sum())
        per_group[g, 2] += int(d.sum())
        per_group[g, 3] = max(int(per_group[g, 3]), int(d.max()) if len(d) else 0)
        group_hist[g] += binned(d)

    for t, d in enumerate(depth):
        outside = np.ones(len(d), bool)
        for k in range(int(iv_off[t]), int(iv_off[t + 1])):
            s, e, g = int(iv_start[k]), int(iv_end[k]), int(iv_group[k])
            inside = d[s:e]
            assert len(inside) == e - s and outside[s:e].all()
            outside[s:e] = False
            per_interval[k] = (int((inside > 0).sum()), int(inside.sum()), int(inside.min()), int(inside.max()))
            take(g, inside)
        take(rest_group, d[outside])
    return per_interval, per_group, group_hist


def g15(a, b):
    return "%.15g" % (a / b) if b else "NaN"


def depth_name(d):
    return ">=1023" if d == BINS - 1 else str(d)


def coverage_text(groups, iv_group, per_group):
    rows = ["Index\tGroup\tRegions\tBases\tCovered\tBreadth\tAlignedBases\tMeanDepth\tMaxDepth"]
    for g, name in enumerate(groups):
        bases, covered, aligned, deepest = (int(x) for x in per_group[g])
        rows.append("\t".join([str(g), name, str(sum(1 for x in iv_group if int(x) == g)), str(bases), str(covered), g15(covered, bases),
                               str(aligned), g15(aligned, bases), str(deepest)]))
    return "\n".join(rows) + "\n"


def histogram_text(groups, group_hist):
    return "Index\tGroup\tDepth\tBases\n" + "".join("%d\t%s\t%s\t%d\n" % (g, name, depth_name(d), int(n)) for g, name in enumerate(groups)
                                                     for d, n in enumerate(group_hist[g]) if n)


def thresholds_text(groups, per_group, group_hist, thresholds):
    rows = ["Index\tGroup\tThreshold\tBases\tFraction\n"]
    for g, name in enumerate(groups):
        for t in thresholds:
            n = sum(int(x) for x in group_hist[g][t:])
            rows.append("%d\t%s\t%d\t%d\t%s\n" % (g, name, t, n, g15(n, int(per_group[g, 0]))))
    return "".join(rows)


def regions_depth_text(names, groups, iv_off, iv_start, iv_end, iv_group, per_interval):
    rows = ["Sequence\tStart\tEnd\tGroup\tCovered\tBreadth\tAlignedBases\tMeanDepth\tMinDepth\tMaxDepth\n"]
    for t, name in enumerate(names):
        for k in range(int(iv_off[t]), int(iv_off[t + 1])):
            covered, aligned, lo, hi = (int(x) for x in per_interval[k])
            span = int(iv_end[k]) - int(iv_start[k])
            rows.append("%s\t%d\t%d\t%s\t%d\t%s\t%d\t%s\t%d\t%d\n" % (name, iv_start[k], iv_end[k], groups[int(iv_group[k])], covered,
                                                                    g15(covered, span), aligned, g15(aligned, span), lo, hi))
    return "".join(rows)
