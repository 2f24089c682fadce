"""--pileup-sites, restated by brute force as the issue words the rule (no line of csrc/mdx_pileup_key.h): every record's
alignment expanded column by column, every column over a site classified, the twelve counters per site summed, the call made
from a site's counters.  The CPU tests hold the header's host build to it, the GPU tests the device stage and the command line's
files.

A record is ``(flag, lib, tid, pos, cigar, seq, qual)``: ``cigar`` [(op, length), ...]; ``seq`` a string of symbols, or — the
packed column's own codes, for what no letter gives — a list of nibbles (1 A, 2 C, 4 T, 8 G); ``qual`` a list of bytes or None
(a record without qualities: 0xFF as its first byte)."""

import numpy as np

from tests.depth_rule import COUNTED, IGNORED, OUTSIDE, classify          # noqa: F401  (a record is counted as --depth counts it)

NAMES = ("A+", "C+", "G+", "T+", "A-", "C-", "G-", "T-", "Deletions", "LowQual", "Other", "Masked")
DELETIONS, LOWQUAL, OTHER, MASKED = 8, 9, 10, 11
BASES = "ACGT"
NIBBLE_BASE = {1: 0, 2: 1, 8: 2, 4: 3}
MASK64 = (1 << 64) - 1
M, I, D, N, S, H, P, EQ, X = range(9)


def query_range(cigar, l_seq):
    """[qs, qe) of SEQ without its terminal soft clips: leading S behind optional H, trailing S in front of optional H, the first
    operation never taken for a trailing one."""
    qs, qe = 0, l_seq
    i = 0
    while i < len(cigar) and cigar[i][0] in (S, H):
        qs += cigar[i][1] if cigar[i][0] == S else 0
        i += 1
    j = len(cigar)
    while j > 1 and cigar[j - 1][0] in (S, H):
        qe -= cigar[j - 1][1] if cigar[j - 1][0] == S else 0
        j -= 1
    return qs, qe


def masked_set(flag, cigar, l_seq, k5, k3):
    """The SEQ indices inside the first ``k5`` query bases of the molecule's 5' end or the last ``k3`` of its 3' end."""
    qs, qe = query_range(cigar, l_seq)
    if qe <= qs:
        return set()
    molecule = list(range(qs, qe))
    if flag & 0x10:
        molecule.reverse()              # 5' to 3'
    return set(molecule[:min(k5, len(molecule))]) | set(molecule[len(molecule) - min(k3, len(molecule)):])


def columns(pos, cigar):
    """The alignment column by column: (reference position or None, SEQ index or None, op)."""
    at, q = pos, 0
    for op, length in cigar:
        for _ in range(length):
            if op in (M, EQ, X):
                yield at, q, op
                at, q = at + 1, q + 1
            elif op in (D, N):
                yield at, None, op
                at += 1
            elif op in (I, S):
                yield None, q, op
                q += 1


def symbol(seq, q):
    """0 .. 3 for exactly A C G T, None for anything else — a SEQ index beyond the record's SEQ too."""
    if q >= len(seq):
        return None
    s = seq[q]
    if isinstance(s, str):
        return BASES.index(s) if s in BASES else None
    return NIBBLE_BASE.get(int(s))


def has_qualities(seq, qual):
    return qual is not None and len(seq) > 0 and len(qual) > 0 and qual[0] != 0xFF


def site_classes(record, sites_of_tid, k5=0, k3=0, min_qual=0, fold_q=0):
    """{position: counter} of the sites the counted record adds to.  ``fold_q``: the --min-basequal of a MDX_SEQ_4BITQ column — a
    base of a record with qualities whose quality is below it is stored as a symbol that is no base."""
    flag, lib, tid, pos, cigar, seq, qual = record
    masked = masked_set(flag, cigar, len(seq), k5, k3)
    with_qual = has_qualities(seq, qual)
    out = {}
    for at, q, op in columns(pos, cigar):
        if at is None or at not in sites_of_tid:
            continue
        if op == D:
            out[at] = DELETIONS
        elif op == N:
            continue
        elif q in masked:
            out[at] = MASKED
        else:
            base = symbol(seq, q)
            if base is not None and fold_q and with_qual and qual[q] < fold_q:
                base = None
            if base is None:
                out[at] = OTHER
            elif with_qual and qual[q] < min_qual:
                out[at] = LOWQUAL
            else:
                out[at] = base + (4 if flag & 0x10 else 0)
    return out


def brute(records, n_libraries, lengths, sites, k5=0, k3=0, min_qual=0, fold_q=0):
    """``sites``: (tid, 0-based position) in (tid, position) order -> (uint32 [sites][12], dict of the records counted, outside,
    over at least one site, and the pairs)."""
    index = {site: g for g, site in enumerate(sites)}
    by_tid = {}
    for t, p in sites:
        by_tid.setdefault(t, set()).add(p)
    counters = np.zeros((len(sites), 12), np.uint32)
    counts = dict(counted=0, outside=0, over_a_site=0, pairs=0)
    for record in records:
        flag, lib, tid, pos, cigar = record[:5]
        kind = classify(flag, lib, tid, pos, cigar, n_libraries, lengths)
        if kind == OUTSIDE:
            counts["outside"] += 1
        if kind != COUNTED:
            continue
        counts["counted"] += 1
        mine = by_tid.get(tid, set())
        span = sum(ln for op, ln in cigar if op in (M, D, N, EQ, X))
        pairs = sum(1 for p in range(pos, pos + span) if p in mine) if len(mine) < span else sum(1 for p in mine if pos <= p < pos + span)
        counts["pairs"] += pairs
        counts["over_a_site"] += 1 if pairs else 0
        for p, cls in site_classes(record, mine, k5, k3, min_qual, fold_q).items():
            counters[index[(tid, p)], cls] += 1
    return counters, counts


def z_of(seed, tid, p):
    z = (seed + 0x9E3779B97F4A7C15 * ((((tid & 0xFFFFFFFF) << 32) | (p & 0xFFFFFFFF)) + 1)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def call(row, mode, seed, tid, p, min_depth=1, alleles=None, single_strand=False):
    """The call of a site from its twelve counters: a letter of ACGT or N.  ``alleles``: (ref, alt) as letters, or None."""
    plus, minus = [int(x) for x in row[0:4]], [int(x) for x in row[4:8]]
    if alleles is not None and single_strand:
        if set(alleles) == {"C", "T"}:
            plus = [0, 0, 0, 0]
        if set(alleles) == {"G", "A"}:
            minus = [0, 0, 0, 0]
    e = [a + b for a, b in zip(plus, minus)]
    if alleles is not None:
        e = [n if BASES[b] in alleles else 0 for b, n in enumerate(e)]
    total = sum(e)
    if total < max(1, min_depth):
        return "N"
    z = z_of(seed, tid, p)
    if mode == "majority":
        best = max(e)
        tied = [b for b in range(4) if e[b] == best]
        return BASES[tied[z % len(tied)]]
    draw, cum = z % total, 0
    for b in range(4):
        cum += e[b]
        if cum > draw:
            return BASES[b]
    raise AssertionError("unreachable")


def calls(counters, sites, mode, seed, min_depth=1, alleles=None, single_strand=False):
    if mode == "none":
        return ["."] * len(sites)
    return [call(counters[g], mode, seed, t, p, min_depth, None if alleles is None else alleles[g], single_strand) for g, (t, p) in enumerate(sites)]


def depths(counters):
    return np.asarray(counters, np.uint32)[:, :8].sum(axis=1, dtype=np.uint64).astype(np.uint32)


def refbases(ref_seqs, sites):
    """The reference's letter at every site in upper case, N for one that is not A, C, G or T (``ref_seqs``: bytes per sequence)."""
    return [chr(ref_seqs[t][p]).upper() if chr(ref_seqs[t][p]).upper() in BASES else "N" for t, p in sites]


def g15(x):
    return "%.15g" % x


def pileup_text(names, sites, ids, alleles, refbase, counters, call_letters):
    """pileup.tsv as the issue words it; ``call_letters`` None: no Call column."""
    rows = ["\t".join(["Sequence", "Position", "Id", "Ref", "Alt", "RefBase"] + list(NAMES) + ["Depth"] + (["Call"] if call_letters is not None else []))]
    depth = depths(counters)
    for g, (t, p) in enumerate(sites):
        ref, alt = alleles[g] if alleles is not None else ("", "")
        row = [names[t], str(p + 1), ids[g] if ids is not None else ".", ref or ".", alt or ".", refbase[g]]
        row += [str(int(x)) for x in counters[g]] + [str(int(depth[g]))]
        rows.append("\t".join(row + ([call_letters[g]] if call_letters is not None else [])))
    return "\n".join(rows) + "\n"


def summary_text(path, min_qual, k5, k3, mode, seed, min_depth, single_strand, counters, call_letters, counts):
    depth = depths(counters).astype(np.int64)
    n = len(depth)
    called = sum(1 for c in call_letters if c in BASES) if call_letters is not None else 0
    head = ["SitesFile", "MinBaseQual", "MaskEnds", "Call", "Seed", "MinDepth", "SingleStrandMode", "Sites", "Covered", "Called", "SumDepth", "MeanDepth",
            "RecordsCounted", "RecordsOutside", "RecordsOverASite", "Pairs", "Deletions", "LowQual", "Other", "Masked"]
    row = [str(path), str(min_qual), "%d,%d" % (k5, k3), mode, str(seed), str(min_depth), str(int(single_strand)), str(n), str(int((depth >= 1).sum())),
           str(called), str(int(depth.sum())), g15(int(depth.sum()) / n), str(counts["counted"]), str(counts["outside"]), str(counts["over_a_site"]),
           str(counts["pairs"])] + [str(int(np.asarray(counters)[:, q].astype(np.uint64).sum())) for q in (8, 9, 10, 11)]
    return "\t".join(head) + "\n" + "\t".join(row) + "\n"


def log_line(mode, seed, counters, call_letters, counts):
    depth = depths(counters).astype(np.int64)
    n, covered = len(depth), int((depth >= 1).sum())
    called = sum(1 for c in call_letters if c in BASES) if call_letters is not None else 0
    how = "%s, seed %d" % (mode, seed) if mode != "none" else "none"
    return ("Pileup: %d sites, %d covered (%s %%), %d called (%s), mean depth %s at sites; %d of %d records over a site; %d records outside "
            "their sequence" % (n, covered, "%.4g" % (100.0 * covered / n), called, how, "%.6g" % (int(depth.sum()) / n), counts["over_a_site"],
                                counts["counted"], counts["outside"]))
