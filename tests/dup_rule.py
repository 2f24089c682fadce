"""--remove-duplicates, restated by brute force: per record its signature as the issue words the rule (not as
csrc/mdx_dup_key.h packs it), then a dict of first occurrences in file order.  The CPU tests hold the header's host build to
it, the GPU tests the flags ``mdx_dedup_mark`` leaves, the counters and the histogram."""

import collections
import struct

import numpy as np

REF_OPS = (0, 2, 3, 7, 8)          # M D N = X
CLIP_OPS = (4, 5)                  # S H
IGNORED, EXAMINED, PAIRED, OTHER = 0, 1, 2, 3
BINS = 1024


def signature(flag, lib, tid, pos, cigar, n_libraries, ends="both"):
    """(kind, signature or None) of one record; ``cigar``: [(op, length), ...]."""
    if flag & 0xF04 or lib >= n_libraries:
        return IGNORED, None
    if flag & 0x1:
        return PAIRED, None
    if tid < 0 or pos < 0:
        return OTHER, None
    span = sum(ln for op, ln in cigar if op in REF_OPS)
    if span < 1:
        return OTHER, None
    lead = 0
    for op, ln in cigar:
        if op not in CLIP_OPS:
            break
        lead += ln
    trail = 0
    for op, ln in reversed(cigar):
        if op not in CLIP_OPS:
            break
        trail += ln
    left, right = pos - lead, pos + span - 1 + trail
    if left < -2**31 or right > 2**32 - 1:
        return OTHER, None
    strand = flag & 0x10
    if ends == "both":
        return EXAMINED, (lib, tid, strand, left, right)
    return EXAMINED, (lib, tid, strand, right if strand else left)


def brute(records, n_libraries, ends="both"):
    """``records``: an iterable of (flag, lib, tid, pos, cigar) in file order -> (duplicate mask, counters [n_libraries][4] =
    examined, duplicates, paired, other, histogram [n_libraries][1024])."""
    records = list(records)
    dup = np.zeros(len(records), bool)
    counts = np.zeros((n_libraries, 4), np.uint64)
    seen = collections.Counter()
    for i, (flag, lib, tid, pos, cigar) in enumerate(records):
        kind, sig = signature(flag, lib, tid, pos, cigar, n_libraries, ends)
        if kind == IGNORED:
            continue
        counts[lib, {EXAMINED: 0, PAIRED: 2, OTHER: 3}[kind]] += 1
        if kind == EXAMINED:
            dup[i] = sig in seen
            counts[lib, 1] += int(dup[i])
            seen[sig] += 1
    hist = np.zeros((n_libraries, BINS), np.uint64)
    for sig, c in seen.items():
        hist[sig[0], min(c, BINS) - 1] += 1
    return dup, counts, hist


def columns(records):
    """The records as the columns of a batch: flag, lib, tid, pos, cigar_off, cigar (BAM's length << 4 | op)."""
    records = list(records)
    flag = np.array([r[0] for r in records], np.uint16)
    lib = np.array([r[1] for r in records], np.uint16)
    tid = np.array([r[2] for r in records], np.int32)
    pos = np.array([r[3] for r in records], np.int32)
    off = np.zeros(len(records) + 1, np.uint32)
    off[1:] = np.cumsum([len(r[4]) for r in records])
    cigar = np.array([ln << 4 | op for r in records for op, ln in r[4]], np.uint32)
    return flag, lib, tid, pos, off, cigar


POOL = np.random.default_rng(3).integers(0, 256, 1 << 16, dtype=np.uint8).tobytes()


def body(flag, tid, pos, cigar, rg=None, salt=0, mapq=60):
    """A BAM record without its block_size: as many bases as the CIGAR's query has, an RG:Z tag for ``rg``.  Name, SEQ and
    QUAL vary with ``salt`` — nothing the rule looks at, and bytes DEFLATE cannot shrink, so a few thousand records fill slabs."""
    n_bases = sum(ln for op, ln in cigar if op in (0, 1, 4, 7, 8))
    o = (salt * 131) % (len(POOL) - 2 * n_bases - 16)
    name = b"r%d" % salt
    ops = b"".join(struct.pack("<I", ln << 4 | op) for op, ln in cigar)
    out = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, n_bases, -1, -1, 0)
    out += name + b"\0" + ops + POOL[o:o + (n_bases + 1) // 2] + bytes(c & 0x3F for c in POOL[o + n_bases:o + 2 * n_bases])
    if rg is not None:
        out += b"RGZ" + rg.encode() + b"\0"
    return out
