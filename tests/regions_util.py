"""Helpers of the region tests (``--regions`` / ``--region-groups``, include/mdx.h ``mdx_set_strata_regions``): a record's
group by brute force in numpy, the classes of records at a region's edges, and the region set of the grid test.

Nothing here uses the product's parser or its key: regions are plain lists of ``(tid, start, end, group)`` as the test wrote
them (unmerged, in any order), a record is compared against every region of its sequence."""

import numpy as np

REF_OPS = (0, 2, 3, 7, 8)            # M D N = X consume the reference
ALIGNED_OPS = (0, 7, 8)              # ... of which these are aligned bases
CLASSES = ("ends at a start", "starts at an end", "one base on the left", "one base on the right", "contains a region",
           "two groups", "only through D or N", "only a soft clip reaches", "region-less sequence")


def _sum_ops(batch, ops, which="all"):
    """Per record: the summed length of its CIGAR operations whose code is in ``ops`` (``which``: all of them, or only
    the run of such operations at the record's ``head`` or ``tail``, hard clips skipped)."""
    n = batch.n
    code, length = batch.cigar & 15, (batch.cigar >> 4).astype(np.int64)
    if which == "all":
        w = np.where(np.isin(code, ops), length, 0)
        padded = np.concatenate([w, [0]])
        total = np.add.reduceat(padded, batch.cigar_off[:-1].astype(np.int64))
        return np.where(batch.cigar_off[1:] > batch.cigar_off[:-1], total, 0)
    out = np.zeros(n, np.int64)
    for i in range(n):
        c = list(zip(code[batch.cigar_off[i]:batch.cigar_off[i + 1]], length[batch.cigar_off[i]:batch.cigar_off[i + 1]]))
        for op, ln in (c if which == "head" else reversed(c)):
            if op == 5:
                continue
            if op not in ops:
                break
            out[i] += ln
    return out


def record_end(batch, ops=REF_OPS):
    """``pos + max(1, reference bases)`` of every record (htslib's ``bam_endpos``)."""
    return batch.pos.astype(np.int64) + np.maximum(1, _sum_ops(batch, ops))


def overlaps(pos, end, regions_of_tid):
    """bool [records][regions]: the record [pos, end) and the region share a base."""
    r = np.asarray(regions_of_tid, np.int64).reshape(-1, 4)
    return (r[None, :, 1] < end[:, None]) & (r[None, :, 2] > pos[:, None])


def brute_group(batch, regions, n_contig, rest):
    """The group of every record: that of the overlapping region that begins first, ``rest`` where there is none."""
    pos, end = batch.pos.astype(np.int64), record_end(batch)
    group = np.full(batch.n, rest, np.int64)
    for t in range(n_contig):
        r = np.asarray(sorted(x for x in regions if x[0] == t), np.int64).reshape(-1, 4)       # by start
        idx = np.nonzero(batch.tid == t)[0]
        if not len(r) or not len(idx):
            continue
        hit = overlaps(pos[idx], end[idx], r)
        group[idx[hit.any(axis=1)]] = r[hit.argmax(axis=1), 3][hit.any(axis=1)]
    return group


def edge_classes(batch, regions, n_contig, rest):
    """{class name: indices of the kept records in it} (``CLASSES``), from the brute-force assignment."""
    pos, end = batch.pos.astype(np.int64), record_end(batch)
    aligned_end = batch.pos.astype(np.int64) + np.maximum(1, _sum_ops(batch, ALIGNED_OPS))
    clip_lo = pos - _sum_ops(batch, (4,), "head")
    clip_hi = end + _sum_ops(batch, (4,), "tail")
    kept = (batch.flag & 0xF04) == 0
    found = {name: [] for name in CLASSES}
    with_regions = {x[0] for x in regions}
    for t in range(n_contig):
        idx = np.nonzero((batch.tid == t) & kept)[0]
        if t not in with_regions:
            found["region-less sequence"].extend(idx.tolist())
            continue
        r = np.asarray(sorted(x for x in regions if x[0] == t), np.int64).reshape(-1, 4)
        p, e = pos[idx][:, None], end[idx][:, None]
        hit = overlaps(pos[idx], end[idx], r)
        none, one = ~hit.any(axis=1), hit.sum(axis=1) == 1
        start, stop, grp = r[None, :, 1], r[None, :, 2], r[None, :, 3]
        sel = {
            "ends at a start": none & (e == start).any(axis=1),
            "starts at an end": none & (p == stop).any(axis=1),
            "one base on the left": one & (hit & (e == start + 1) & (p < start)).any(axis=1),
            "one base on the right": one & (hit & (p == stop - 1) & (e > stop)).any(axis=1),
            "contains a region": ((p < start) & (e > stop)).any(axis=1),
            "two groups": np.asarray([len(set(grp[0][h])) > 1 for h in hit], bool).reshape(len(idx)),
            "only through D or N": hit.any(axis=1) & ~overlaps(pos[idx], aligned_end[idx], r).any(axis=1),
            "only a soft clip reaches": none & overlaps(clip_lo[idx], clip_hi[idx], r).any(axis=1),
        }
        for name, mask in sel.items():
            found[name].extend(idx[mask].tolist())
    return found


def bed_text(regions, names, group_names=None):
    """The BED text of ``regions`` (``group_names``: a fourth column)."""
    return "".join("%s\t%d\t%d%s\n" % (names[t], s, e, "" if group_names is None else "\t" + group_names[g])
                   for t, s, e, g in regions)


def merged_figures(regions, lengths, n_groups):
    """(regions, bases) per group after merging overlapping and abutting regions of one group, by brute force over a
    per-base map; the last group — ``*`` — has no regions and the bases nothing covers."""
    n_regions, n_bases = [0] * n_groups, [0] * n_groups
    for t, ln in enumerate(lengths):
        owner = np.full(ln + 1, -1, np.int64)
        for tt, s, e, g in regions:
            if tt == t:
                owner[s:e] = g
        for g in range(n_groups - 1):
            mine = (owner == g).astype(np.int8)
            n_bases[g] += int(mine.sum())
            n_regions[g] += int((np.diff(np.concatenate([[0], mine])) == 1).sum())
        n_bases[n_groups - 1] += int((owner[:ln] == -1).sum())
    return n_regions, n_bases


# ---------------------------------------------------------------------- the grid's regions over tests.test_gpu_strata.genome5()
GRID_GROUPS = ["cap_a", "cap_b", "cap_c", "*"]
GRID_LENGTHS = (9000, 5000, 3000, 2500, 2000)        # chr1, chr2, chrM (no regions), scaf/1:a, chr* (wholly covered)


def grid_regions():
    """About 40 regions of 1 to 900 bases in three groups: sequence 2 has none, sequence 4 is wholly covered (abutting
    regions), some regions abut one of another group, some are a single base."""
    rng = np.random.default_rng(5)
    spans = [1, 1, 2, 3, 7, 30, 64, 150, 400, 900]
    out = []
    for t, n in ((0, 17), (1, 10), (3, 7)):
        at = 40
        for k in range(n):
            ln = spans[int(rng.integers(len(spans)))]
            if at + ln > GRID_LENGTHS[t] - 40:
                break
            out.append((t, at, at + ln, int(rng.integers(3))))
            # a third of the regions abut their successor, the others leave a gap shorter or longer than a read
            at += ln + (0 if k % 3 == 1 else int(rng.integers(1, 600)))
    out += [(4, 0, 700, 0), (4, 700, 1400, 1), (4, 1400, 1401, 2), (4, 1401, 2000, 1)]
    # (abutting regions of one group would be one region: give the successor another group, so that what the test lists is
    # what the product holds after merging, and every abutting pair is a boundary between two groups)
    fixed = []
    for t, s, e, g in out:
        if fixed and fixed[-1][0] == t and fixed[-1][2] == s and fixed[-1][3] == g:
            g = (g + 1) % 3
        fixed.append((t, s, e, g))
    return fixed
